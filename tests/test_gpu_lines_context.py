"""The line filter with context lines (sre_hip_filter_lines_context): grep -A / -B / -C from one device buffer to another.

Expected output is pure Python: the split rule of line mode, the oracle's verdict on every line, the dilation rule of
the header (line i is selected when it is matched, or some matched j has j < i <= j + after or i < j <= i + before),
joined with delimiters.  Every output and index buffer has the filter tests' guard bytes and 0xA5 fill; every check
asserts the guards and everything at or beyond out_bytes.
"""
import ctypes
import random

import pytest

import sregex_amd as S
from test_gpu_lines import Expect, split_lines, upload_at
from test_gpu_lines_filter import HEADLINE, ROUTES, Out, cut, download, random_lines, small_buffer
from test_gpu_nfa_wide import WIDE

pytestmark = pytest.mark.gpu

SIZE_MAX = (1 << 64) - 1
N_EDGE = 3 * 1024 + 17
CONTEXT, GROUP = 1, 2


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def dilate(matched, before, after):
    """the selected lines: the nearest matched line at or in front of i is at most `after` lines away, or the nearest one
    at or behind it at most `before`"""
    n = len(matched)
    sel, last = [False] * n, None
    for i in range(n):
        last = i if matched[i] else last
        sel[i] = last is not None and i - last <= after
    last = None
    for i in reversed(range(n)):
        last = i if matched[i] else last
        sel[i] = sel[i] or (last is not None and last - i <= before)
    return sel


def by_definition(matched, before, after):
    js = [j for j, m in enumerate(matched) if m]
    return [matched[i] or any(j < i <= j + after or i < j <= i + before for j in js) for i in range(len(matched))]


def test_the_python_dilation_is_the_definition():
    m = [k in (0, 7, 8, 30, 59) for k in range(60)]
    for b, a in [(0, 0), (1, 0), (0, 1), (2, 3), (3, 2), (10, 11), (11, 11), (60, 0), (0, 61), (SIZE_MAX, SIZE_MAX)]:
        assert dilate(m, b, a) == by_definition(m, b, a)


class Case:
    """one source buffer on the device with the oracle's verdict on each of its lines"""

    def __init__(self, sc, exp, data, mode, delim=0x0A, src_off=0):
        self.sc, self.lib, self.data, self.delim, self.src_off = sc, sc.lib, data, delim, src_off
        self.lines = split_lines(data, delim)
        self.hits = [exp.record(data[st:st + n], mode)[0] != S.SRE_DECLINED for st, n in self.lines]
        self.src = upload_at(data, src_off)
        self.ptr = self.src.ptr + src_off

    def free(self):
        self.src.free()

    def expected(self, before, after, invert=False):
        """(rows [(line, start, len, output offset, flags)] of all selected lines, matched lines, groups)"""
        matched = [h != invert for h in self.hits]
        sel = dilate(matched, before, after)
        rows, o = [], 0
        for i, (st, n) in enumerate(self.lines):
            if sel[i]:
                flags = (0 if matched[i] else CONTEXT) | (GROUP if i == 0 or not sel[i - 1] else 0)
                rows.append((i, st, n, o, flags))
                o += n + 1
        return rows, sum(matched), sum(1 for r in rows if r[4] & GROUP)

    def run(self, before, after, invert=False, dst_off=0, out_cap=None, index_cap=None, null_out=False):
        """one call, checked in full; returns (info, output bytes, index rows)"""
        d = bytes([self.delim])
        rows, nmatched, ngroups = self.expected(before, after, invert)
        need = sum(r[2] + 1 for r in rows)
        cap = need + 37 if out_cap is None else out_cap
        nwritten, out_bytes = cut([r[:3] for r in rows], cap)
        want = b"".join(self.data[st:st + n] + d for _, st, n, _, _ in rows[:nwritten])
        assert len(want) == out_bytes
        icap = len(rows) + 3 if index_cap is None else index_cap
        out = Out(self.lib, cap, dst_off)
        idx = Out(self.lib, icap * 40, 0)
        try:
            info = self.sc.filter_lines_context(self.ptr, len(self.data), None if null_out else out.ptr, cap, before, after,
                                                self.delim, invert, idx.ptr if icap else None, icap)
            assert info == S.ContextInfo(len(self.lines), nmatched, len(rows), ngroups, need, nwritten, out_bytes), \
                (info, nmatched, len(rows), ngroups, need, before, after)
            out.check(want)
            nrows = min(icap, nwritten)
            raw = (ctypes.c_int64 * (5 * nrows)).from_buffer_copy(download(self.lib, idx.ptr, 40 * nrows)) if nrows else []
            got = [tuple(raw[5 * r:5 * r + 5]) for r in range(nrows)]
            assert got == rows[:nrows], ([(g, w) for g, w in zip(got, rows) if g != w][:3], before, after)
            idx.check(download(self.lib, idx.ptr, 40 * nrows))      # nothing behind the rows, nothing around the index
        finally:
            out.free()
            idx.free()
        return info, want, rows[:nrows]


def headline(pool, mode=S.HIP_PIKE_FIRST, engine=S.ENGINE_AUTO):
    re = S.parse(pool, HEADLINE)
    prog = S.compile(pool, re)
    return S.Scanner(pool, prog, mode, engine), Expect(prog, re.ncaps, key=("filter", tuple(HEADLINE)))


def edge_buffer(spots, final_delim, n=N_EDGE):
    """n lines of 0 .. 40 bytes that cannot match, a match planted in the lines `spots`; empty lines beside the edges of
    the waves and workgroups, so that context lines are empty too"""
    rng = random.Random(41)
    words = [b""] + [bytes(rng.choice(b"xyw .") for _ in range(rng.randrange(0, 41))) for _ in range(47)]
    lines = [rng.choice(words) for _ in range(n)]
    for k in (1, 2, 254, 257, 1022, 1025, n - 2):
        lines[k] = b""
    for s in spots:
        lines[s] = b"ab q@q.q" if s % 2 else b"q@q.q"
    return b"\n".join(lines) + (b"\n" if final_delim else b"")


# ------------------------------------------------------------------ 1. block and wave edges

EDGES = [0, 255, 256, 1023, 1024, N_EDGE - 1]
WINDOWS = [0, 1, 3, 4, 63, 64, 255, 256, 1023, 1024, 1025, N_EDGE - 1, N_EDGE, N_EDGE + 1]
ASYMMETRIC = [(1, 0), (0, 1), (3, 64), (256, 4), (0, 1025), (1024, 0), (N_EDGE + 1, 1), (63, N_EDGE), (1 << 63, 0), (0, SIZE_MAX)]


@pytest.mark.parametrize("spots", [[s] for s in EDGES] + [EDGES], ids=[str(s) for s in EDGES] + ["together"])
def test_block_and_wave_edges(gpu, spots):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        assert sc.engine == S.ENGINE_SCAN
        cases = [Case(sc, exp, edge_buffer(spots, final), S.HIP_PIKE_FIRST) for final in (False, True)]
        try:
            assert all(len(c.lines) == N_EDGE and sum(c.hits) == len(spots) for c in cases)
            for k, (b, a) in enumerate([(w, w) for w in WINDOWS] + ASYMMETRIC):
                info, want, rows = cases[k % 2].run(b, a)
                assert info.nmatched == len(spots)
                # empty lines came out as context, each with its delimiter
                if b >= 3 and a >= 3:
                    assert any(r[2] == 0 and r[4] & CONTEXT for r in rows)
            assert sc.last_lines_device == 1
        finally:
            for c in cases:
                c.free()


# ------------------------------------------------------------------ 2. the carry across a workgroup without a match

def test_carry_across_an_empty_block(gpu):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        for spot, b, a in [(5, 0, 2500), (N_EDGE - 3, 2500, 0)]:
            c = Case(sc, exp, edge_buffer([spot], True), S.HIP_PIKE_FIRST)
            try:
                info, _, rows = c.run(b, a)
                assert (info.nmatched, info.nselected, info.ngroups) == (1, 2501, 1)
                assert [r[0] for r in rows] == list(range(min(spot, spot - b), max(spot, spot + a) + 1))
            finally:
                c.free()


# ------------------------------------------------------------------ 3. real batch cuts

def test_real_batch_cuts(gpu, monkeypatch):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        c = Case(sc, exp, edge_buffer([0, 650, 699, 700, 1399, 1500, 2800, N_EDGE - 1], False), S.HIP_PIKE_FIRST, src_off=3)
        try:
            windows = [(2, 3), (60, 0), (0, 60), (800, 800)]
            one = [c.run(b, a, dst_off=5) for b, a in windows]
            assert sc.last_line_batches == 1
            monkeypatch.setenv("SRE_HIP_LINES_BATCH", "700")        # cuts inside workgroups, contexts across batches
            for (b, a), (info1, want1, rows1) in zip(windows, one):
                info, want, rows = c.run(b, a, dst_off=5)
                assert sc.last_line_batches == 5 > 1
                assert (info, want, rows) == (info1, want1, rows1)
        finally:
            c.free()


# ------------------------------------------------------------------ 4. every route

@pytest.mark.parametrize("name,pats,mode,engine,routed,device", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route(gpu, monkeypatch, name, pats, mode, engine, routed, device):
    data = random_lines(5)
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps, key=("filter", tuple(pats)))
        sc = S.Scanner(pool, prog, mode, engine)
        assert sc.engine == routed
        if name.startswith("nfa-wide"):
            assert sc.nfa_bits == WIDE[1][1]
        c = Case(sc, exp, data, mode, src_off=3)
        try:
            assert 0 < sum(c.hits) < len(c.lines) == 2000
            info, want, _ = c.run(2, 3, dst_off=5)
            assert sc.last_lines_device == device and sc.last_line_batches >= 1
            assert info.nmatched < info.nselected <= info.nlines and info.ngroups >= 1
            assert sc.last_short_lines > 0 or name not in ("nfa-thompson", "nfa-first")
            if sc.last_short_lines > 0:
                monkeypatch.setenv("SRE_HIP_LINES_SHORT_MAX", "0")      # every line through the tier's set pass
                info0, want0, _ = c.run(2, 3, dst_off=5)
                assert sc.last_short_lines == 0 and sc.last_lines_device == 1
                assert (info0, want0) == (info, want)
        finally:
            c.free()


# ------------------------------------------------------------------ 5. grep -v with context

def test_invert_with_context(gpu):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        # most lines match, so that the inverted rule picks a few and the context lines are matching lines
        lines = [b"a@b.c %d" % (k % 7) for k in range(1500)]
        for k in (0, 1, 400, 402, 1023, 1024, 1026, 1499):
            lines[k] = b"nothing here" if k % 2 else b""
        for final in (False, True):
            c = Case(sc, exp, b"\n".join(lines) + (b"\n" if final else b""), S.HIP_PIKE_FIRST)
            try:
                info, _, rows = c.run(1, 1, invert=True)
                assert info.nmatched == 8 and [r[0] for r in rows] == [0, 1, 2, 399, 400, 401, 402, 403, 1022, 1023, 1024, 1025,
                                                                       1026, 1027, 1498, 1499]
                assert info.ngroups == 4
                c.run(0, 0, invert=True)
                c.run(3, 0, invert=True)
                c.run(0, 700, invert=True)
            finally:
                c.free()


# ------------------------------------------------------------------ 6. without context: the filter itself

def test_zero_context_equals_the_filter(gpu):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        inputs = [small_buffer(9, final_delim=True), small_buffer(10), edge_buffer([0, 255, 256, 1024, 2000, 2001], False)]
        for data in inputs:
            c = Case(sc, exp, data, S.HIP_PIKE_FIRST, src_off=1)
            for invert in (False, True):
                out = Out(gpu, len(data) + len(c.lines) + 8, 7)
                idx = Out(gpu, 32 * (len(c.lines) + 1), 0)
                try:
                    f = sc.filter_lines(c.ptr, len(data), out.ptr, out.cap, invert=invert, index_ptr=idx.ptr,
                                        index_cap=len(c.lines) + 1)
                    body = download(gpu, out.ptr, f.out_bytes)
                    out.check(body)
                    raw = (ctypes.c_int64 * (4 * f.nwritten)).from_buffer_copy(download(gpu, idx.ptr, 32 * f.nwritten))
                    frows = [tuple(raw[4 * r:4 * r + 4]) for r in range(f.nwritten)]
                    info, want, rows = c.run(0, 0, invert=invert, dst_off=7)
                    assert want == body and f.nselected > 0
                    assert (info.nlines, info.nselected, info.need_bytes, info.nwritten, info.out_bytes) == tuple(f)
                    assert info.nmatched == info.nselected
                    assert [r[:4] for r in rows] == frows and all(r[4] & CONTEXT == 0 for r in rows)
                finally:
                    out.free()
                    idx.free()
            c.free()


# ------------------------------------------------------------------ 7. truncation

def test_truncation(gpu):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        c = Case(sc, exp, edge_buffer([40, 1030], True, n=1100), S.HIP_PIKE_FIRST, src_off=1)
        try:
            rows, _, _ = c.expected(6, 9)
            need = sum(r[2] + 1 for r in rows)
            assert len(rows) == 32 and any(r[2] == 0 for r in rows)
            # a cut inside the context run behind the first match: every byte position around the end of a context line
            k = next(k for k in range(8, 16) if rows[k][2] > 1)
            assert rows[k][4] & CONTEXT and rows[k - 1][4] & CONTEXT
            end = rows[k][3] + rows[k][2] + 1
            for dst_off in (0, 5):
                for cap, nwritten in [(need, 32), (need - 1, 31), (end, k + 1), (end - 1, k), (end - 2, k), (end + 1, None),
                                      (rows[k][3], k), (rows[0][2], 0), (0, 0)]:
                    info, _, _ = c.run(6, 9, dst_off=dst_off, out_cap=cap)
                    assert nwritten is None or info.nwritten == nwritten
                    assert info.need_bytes == need and info.nselected == 32 and info.ngroups == 2 and info.out_bytes <= cap
            # a sizing call: no output buffer at all
            info, _, _ = c.run(6, 9, out_cap=0, null_out=True, index_cap=0)
            assert info == S.ContextInfo(1100, 2, 32, 2, need, 0, 0)
            # fewer index rows than written lines, and no index at all
            for icap in (0, 1, 17, 31):
                info, _, got = c.run(6, 9, index_cap=icap)
                assert info.nwritten == 32 and len(got) == icap
            info, _, got = c.run(6, 9, out_cap=need // 2, index_cap=3)
            assert 3 < info.nwritten < 32 and len(got) == 3
        finally:
            c.free()


# ------------------------------------------------------------------ 8. index flags and counts

def test_index_flags_and_counts(gpu):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        c = Case(sc, exp, edge_buffer([100, 103, 110, 111, 130, 1020, 1030], False, n=1200), S.HIP_PIKE_FIRST)
        try:
            for b, a, groups, selected in [
                (0, 0, 6, 7),               # 110 and 111 are one group already
                (2, 2, 5, 29),              # the contexts of 100 and 103 overlap: every line once
                (1, 1, 5, 19),              # ... are adjacent, 101 | 102: one group
                (0, 2, 5, 19),
                (9, 8, 3, 75),              # 111 + 8 and 130 - 9 leave line 120 out: two groups
                (9, 9, 2, 78),              # 120 | 121: they merge
                (0, 17, 3, 75),             # the same from one side
                (0, 18, 2, 78),
                (18, 0, 2, 78),
                (4, 4, 4, 47),              # 1020 + 4 and 1030 - 4 leave 1025 out, across the workgroup edge 1023 | 1024
                (5, 4, 3, 51),
                (4, 5, 3, 51),
            ]:
                info, _, rows = c.run(b, a)
                assert (info.nmatched, info.ngroups, info.nselected) == (7, groups, selected), (b, a, info)
                assert sum(1 for r in rows if r[4] & GROUP) == groups and sum(1 for r in rows if not r[4] & CONTEXT) == 7
        finally:
            c.free()
        # no line matches: every count but nlines is zero and the output is untouched
        c = Case(sc, exp, edge_buffer([], True, n=1100), S.HIP_PIKE_FIRST)
        try:
            for b, a in [(0, 0), (3, 3), (SIZE_MAX, SIZE_MAX)]:
                info, want, _ = c.run(b, a)
                assert info == S.ContextInfo(1100, 0, 0, 0, 0, 0, 0) and want == b""
            # every line matches (inverted): one group, no context bit
            info, _, rows = c.run(5, 5, invert=True)
            assert (info.nmatched, info.nselected, info.ngroups) == (1100, 1100, 1)
            assert [r[4] for r in rows] == [GROUP] + [0] * 1099
        finally:
            c.free()


# ------------------------------------------------------------------ 9. alignments

def test_alignments(gpu):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        data = edge_buffer([3, 500, 1023, 1100], False, n=1300)
        for src_off, dst_off in [(0, 0), (1, 15), (7, 8), (15, 1)]:
            c = Case(sc, exp, data, S.HIP_PIKE_FIRST, src_off=src_off)
            try:
                c.run(4, 7, dst_off=dst_off)
                c.run(300, 0, dst_off=dst_off)
            finally:
                c.free()


# ------------------------------------------------------------------ 10. bad arguments

def test_bad_arguments(gpu):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        data = small_buffer(9)
        src = upload_at(data, 0)
        lines = split_lines(data, 0x0A)
        need = sum(n + 1 for _, n in lines)
        out = Out(gpu, need + 64, 0)
        idx = Out(gpu, 4096, 0)
        info = (ctypes.c_size_t * 7)(*([77] * 7))
        call = gpu.sre_hip_filter_lines_context
        try:
            ALL, INV = S.HIP_LINES_ALL, S.HIP_LINES_INVERT
            for flags, b, a in [(ALL, 1, 0), (ALL, 0, 1), (ALL, 2, 2), (ALL | INV, 0, 0), (ALL | INV, 1, 1), (4, 0, 0), (4, 1, 1),
                                (8 | INV, 1, 0), (-1, 0, 0)]:
                assert call(sc.h, src.ptr, len(data), 0x0A, flags, b, a, out.ptr, out.cap, idx.ptr, 100, info, None) == -1
            # the output overlaps the source
            assert call(sc.h, src.ptr, len(data), 0x0A, 0, 1, 1, src.ptr + 10, 64, None, 0, info, None) == -1
            assert call(sc.h, src.ptr, len(data), 0x0A, 0, 1, 1, src.ptr + len(data) - 1, 64, None, 0, info, None) == -1
            # NULL with a capacity, a delimiter that is no byte
            assert call(sc.h, src.ptr, len(data), 0x0A, 0, 1, 1, None, 64, None, 0, info, None) == -1
            assert call(sc.h, src.ptr, len(data), 0x0A, 0, 1, 1, out.ptr, 64, None, 5, info, None) == -1
            assert call(sc.h, None, len(data), 0x0A, 0, 1, 1, out.ptr, 64, None, 0, info, None) == -1
            assert call(sc.h, src.ptr, len(data), 256, 0, 1, 1, out.ptr, 64, None, 0, info, None) == -1
            assert call(None, src.ptr, len(data), 0x0A, 0, 1, 1, out.ptr, 64, None, 0, info, None) == -1
            assert list(info) == [77] * 7
            out.check(b"")
            idx.check(b"")
            # ALL without context is the filter's ALL; an empty buffer is all zeros
            assert call(sc.h, src.ptr, len(data), 0x0A, ALL, 0, 0, out.ptr, out.cap, idx.ptr, 100, info, None) == 0
            assert list(info) == [len(lines), len(lines), len(lines), 1, need, len(lines), need]
            assert call(sc.h, src.ptr, 0, 0x0A, 0, 3, 3, out.ptr, out.cap, idx.ptr, 100, info, None) == 0
            assert list(info) == [0] * 7
        finally:
            src.free()
            out.free()
            idx.free()
