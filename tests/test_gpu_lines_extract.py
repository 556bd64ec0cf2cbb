"""The line extract (sre_hip_extract_lines): the text of chosen capture groups of every matching line as rows of
separator-delimited fields in a device buffer, with an optional device-side index.

Expected output is pure Python: the split rule of line mode, the oracle's first-match record of every line, and
slicing.  Every output buffer has 64 guard bytes in front and behind and is pre-filled with 0xA5 (the filter test's
Out); every check asserts that the guards and everything at or beyond out_bytes still hold 0xA5.
"""
import ctypes
import random

import pytest

import sregex_amd as S
from test_gpu_lines import Expect, split_lines, upload_at
from test_gpu_lines_filter import Out, download
from test_gpu_nfa_wide import WIDE

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
HEADLINE = [rb"[a-z]+@[a-z]+\.[a-z]+"]
URI = [rb"([a-z]+)://([^/ ]+)(/[^ ?]*)?(\?[^ ]*)?"]
COUNTED = [rb"(?:a|b)*a(?:a|b){7}@"]
DOTTED = [rb"\d{1,3}(\.\d{1,3}){3}"]
BRACKET = [rb"\[([^\]]*)\]"]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


class Program:
    def __init__(self, pool, pats, engine=S.ENGINE_AUTO, mode=FIRST, key=True):
        self.re = S.parse(pool, pats)
        self.prog = S.compile(pool, self.re)
        self.ncaps = self.re.ncaps
        self.exp = Expect(self.prog, self.ncaps, key=("extract", tuple(pats)) if key else None)
        self.sc = S.Scanner(pool, self.prog, mode, engine)


def expected(exp, data, delim, groups, all_lines):
    """[(line, start, len, [(offset in the buffer, length) or None per field])] of the selected lines"""
    out = []
    for i, (st, n) in enumerate(split_lines(data, delim)):
        rec = exp.record(data[st:st + n], FIRST)
        hit = rec[0] != S.SRE_DECLINED
        if not (hit or all_lines):
            continue
        fields = []
        for g in groups:
            a, b = rec[2 + 2 * g], rec[3 + 2 * g]
            fields.append((st + a, b - a) if hit and a >= 0 and b >= a else None)
        out.append((i, st, n, fields))
    return out


def row_text(data, fields, fsep, delim):
    return bytes([fsep]).join(data[f[0]:f[0] + f[1]] if f else b"" for f in fields) + bytes([delim])


def run_extract(sc, exp, data, groups, delim=0x0A, fsep=0x09, src_off=0, dst_off=0, all_lines=False, out_cap=None,
                index_cap=None, null_out=False):
    """one call, checked in full: info, output, guards, index rows; returns (info, output bytes, expected rows)"""
    lib = sc.lib
    K = len(groups)
    sel = expected(exp, data, delim, groups, all_lines)
    texts = [row_text(data, f, fsep, delim) for _, _, _, f in sel]
    need = sum(len(t) for t in texts)
    assert need == sum(sum(f[1] for f in fl if f) + K for _, _, _, fl in sel)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for t in texts:
        if out_bytes + len(t) > cap:
            break
        out_bytes += len(t)
        nwritten += 1
    want = b"".join(texts[:nwritten])
    icap = len(sel) + 3 if index_cap is None else index_cap
    width = 4 + 2 * K
    src = upload_at(data, src_off)
    out = Out(lib, cap, dst_off)
    idx = Out(lib, icap * width * 8, 0)
    try:
        info = sc.extract_lines(src.ptr + src_off, len(data), groups, None if null_out else out.ptr, cap, delim, fsep, all_lines,
                                idx.ptr if icap else None, icap)
        assert info == S.FilterInfo(len(split_lines(data, delim)), len(sel), need, nwritten, out_bytes), (info, len(sel), need)
        out.check(want)
        nrows = min(icap, nwritten)
        rows, o = [], 0
        for (i, st, n, fields), t in zip(sel[:nrows], texts):
            row = [i, st, n, o]
            for f in fields:
                row += list(f) if f else [-1, -1]
            rows.append(tuple(row))
            o += len(t)
        raw = (ctypes.c_int64 * (width * nrows)).from_buffer_copy(download(lib, idx.ptr, 8 * width * nrows)) if nrows else []
        got = [tuple(raw[width * r:width * (r + 1)]) for r in range(nrows)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
        idx.check(download(lib, idx.ptr, 8 * width * nrows))      # nothing behind the rows, nothing around the index
    finally:
        src.free()
        out.free()
        idx.free()
    return info, want, sel


# ------------------------------------------------------------------ 1. the split

def test_split_edges(gpu):
    with S.Pool() as pool:
        for pats in ([rb"a"], [rb"^$|b"]):          # the second matches the empty line
            p = Program(pool, pats, key=False)
            for delim in (0x0A, 0, 255):
                d = bytes([delim])
                for fsep in (0x09, 0):
                    for data in [b"", d, b"a" + d + d + b"b", b"a", d * 5, d * 40 + b"a"]:
                        for all_lines in (False, True):
                            info, _, _ = run_extract(p.sc, p.exp, data, [0], delim, fsep, all_lines=all_lines)
                        if data == b"":
                            assert info == S.FilterInfo(0, 0, 0, 0, 0)
                        assert info.nselected == info.nlines


EMPTY_MATCH_LINES = [b"ab cd", b" x", b"", b"cd ab", b"x", b"b a"]


@pytest.mark.parametrize("delim", [0x0A, ord("a")], ids=["newline", "a"])
def test_an_empty_match_at_either_end_of_the_line(gpu, delim):
    """^ and \\b match the empty string at offset 0 of a line that is not empty, $ at its end.  With the delimiter "a"
    the byte behind a line's end (and the one in front of its start) is a word character, and the line is still its own
    stream: \\b in front of "b cd" and $ behind it match"""
    data = bytes([delim]).join(EMPTY_MATCH_LINES)
    lines = split_lines(data, delim)
    assert sum(1 for _, n in lines if n) >= 5 and any(n == 0 for _, n in lines)
    with S.Pool() as pool:
        for pat, at in [(rb"^", "start"), (rb"$", "end"), (rb"\b", None)]:
            p = Program(pool, [pat], key=False)
            for all_lines in (False, True):
                _, want, sel = run_extract(p.sc, p.exp, data, [0], delim, src_off=1, dst_off=3, all_lines=all_lines)
                if at:
                    # every line matches, with an empty field: the output is one delimiter a line
                    assert [(i, st, n) for i, st, n, _ in sel] == [(i, st, n) for i, (st, n) in enumerate(lines)]
                    assert [f for _, _, _, f in sel] == [[(st + (n if at == "end" else 0), 0)] for st, n in lines]
                    assert want == bytes([delim]) * len(lines)
                elif not all_lines:
                    # a line with a word character has its first boundary in front of its first word
                    word = [(i, st + min(k for k in range(n) if data[st + k:st + k + 1].isalnum()))
                            for i, (st, n) in enumerate(lines) if any(data[st + k:st + k + 1].isalnum() for k in range(n))]
                    assert [(i, f[0]) for i, _, _, f in sel] == [(i, (o, 0)) for i, o in word]
                    assert any(o == lines[i][0] for i, o in word) and any(o > lines[i][0] for i, o in word)


# ------------------------------------------------------------------ 2. alignment and lengths

LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]


def bracketed_buffer(rng):
    """one bracketed field of each of LENGTHS and one of 200 KiB, each at a random position in a line of filler"""
    lines = []
    for n in LENGTHS[:7] + [200 * 1024] + LENGTHS[7:]:
        field = bytes(rng.choice(b"abc[ \t") for _ in range(n))
        fill = bytes(rng.choice(b"xyw ") for _ in range(rng.randrange(0, 80)))
        at = rng.randrange(0, len(fill) + 1)
        lines.append(fill[:at] + b"[" + field + b"]" + fill[at:])
    lines.insert(3, b"no bracket here")
    return b"\n".join(lines)


@pytest.mark.parametrize("groups", [[1], [0, 1], [1, 1, 0]], ids=["g1", "g01", "g110"])
def test_alignment_and_lengths(gpu, groups):
    rng = random.Random(51)
    data = bracketed_buffer(rng)
    with S.Pool() as pool:
        p = Program(pool, BRACKET)
        for src_off in (0, 1, 7, 15):
            for dst_off in (0, 1, 8, 15):
                info, _, sel = run_extract(p.sc, p.exp, data, groups, src_off=src_off, dst_off=dst_off)
                assert info.nselected == len(LENGTHS) + 1 == info.nlines - 1
        # the field lengths are the ones asked for
        assert sorted(f[0][1] for _, _, _, f in expected(p.exp, data, 0x0A, [1], False)) == sorted(LENGTHS + [200 * 1024])


# ------------------------------------------------------------------ 3. unset against empty

URI_LINES = [b"see http://a.b/c?d=e now", b"ftp://host/ and more", b"x://y", b"nothing", b"", b"q://h?x ", b"://no",
             b"abc://abc.cc/ab/c?a=b", b"ab://c/", b"ab://c?", b"a b://cc dd://ee/f"]


def test_unset_against_empty(gpu):
    data = b"\n".join(URI_LINES * 3)
    with S.Pool() as pool:
        p = Program(pool, URI)
        for groups in ([1, 2, 3, 4], [4, 0]):
            for all_lines in (False, True):
                _, _, sel = run_extract(p.sc, p.exp, data, groups, src_off=2, dst_off=3, all_lines=all_lines)
            fields = [f for _, _, _, fl in expected(p.exp, data, 0x0A, [3, 4], False) for f in fl]
            assert None in fields and any(f for f in fields)               # unset and set, both checked in the index rows
        # a group that is set and empty, next to lines where the same group is unset
        q = Program(pool, [rb"x(a*)y|z(b)?"])
        data = b"\n".join([b"xy", b"xaay", b"z", b"zb", b"w", b"--xy--", b"xaaaaaaaaaaaaaaaaay z"])
        _, _, sel = run_extract(q.sc, q.exp, data, [1, 2, 0, 1], fsep=ord(","))
        by_line = {i: f for i, _, _, f in sel}
        assert by_line[0][0] == (1, 0) and by_line[0][1] is None            # x()y: group 1 empty at offset 1, group 2 unset
        assert by_line[2][0] is None and by_line[2][1] is None and by_line[2][2] == (8, 1)
        assert by_line[3][1] == (11, 1) and 4 not in by_line
        # several regexes: the groups are those of the regex that matched
        m = Program(pool, [rb"k=(\d+)", rb"([a-z]+)@([a-z]+)"])
        data = b"\n".join([b"k=12 ab@cd", b"ab@cd k=12", b"none", b"k=", b"zz@y"])
        _, want, _ = run_extract(m.sc, m.exp, data, [1, 2, 0], fsep=ord("|"))
        assert want == b"12||k=12\nab|cd|ab@cd\nzz|y|zz@y\n"


# ------------------------------------------------------------------ 4. every route

PLANTS = [b"ab@ab.ab", b"abaabaabab@", b"1.22.3.4", b"a" + b"ab" * 20 + b"c" + b"q" * 40 + b"@", b"q@q.q", b"10.0.0.255 ",
          b"ab://ab.c/a?1 ", b" x://1.1"]


def random_lines(seed, nlines=2000):
    rng = random.Random(seed)
    lines = []
    for k in range(nlines):
        n = 5000 if k % 400 == 7 else rng.randrange(0, 301)
        line = bytes(rng.choice(b"ab@.1c x") for _ in range(n))
        if rng.random() < 0.3:
            p = rng.choice(PLANTS)
            at = rng.randrange(0, max(1, n - len(p)))
            line = line[:at] + p + line[at + len(p):]
        lines.append(line)
    return b"\n".join(lines)            # (no final delimiter)


ROUTES = [
    ("scan-first-headline", HEADLINE, S.ENGINE_AUTO, S.ENGINE_SCAN, 1),
    ("scan-first-uri", URI, S.ENGINE_AUTO, S.ENGINE_SCAN, 1),
    ("nfa-first", COUNTED, S.ENGINE_NFA, S.ENGINE_NFA, 1),
    ("nfa-first-dotted", DOTTED, S.ENGINE_NFA, S.ENGINE_NFA, 1),
    ("nfa-wide-first", WIDE[1][0], S.ENGINE_NFA, S.ENGINE_NFA, 1),
    ("vm-first", HEADLINE, S.ENGINE_VM, S.ENGINE_VM, 0),
]


@pytest.mark.parametrize("name,pats,engine,routed,device", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route(gpu, name, pats, engine, routed, device):
    data = random_lines(5)
    with S.Pool() as pool:
        p = Program(pool, pats, engine)
        assert p.sc.engine == routed
        if name.startswith("nfa-wide"):
            assert p.sc.nfa_bits == WIDE[1][1]
        groups = [0] + list(range(p.ncaps + 1))
        info, _, _ = run_extract(p.sc, p.exp, data, groups, src_off=3, dst_off=5)
        assert p.sc.last_lines_device == device and p.sc.last_line_batches >= 1
        assert 0 < info.nselected < info.nlines == 2000, info
        info, _, _ = run_extract(p.sc, p.exp, data, groups, src_off=3, dst_off=5, all_lines=True)
        assert p.sc.last_lines_device == device
        assert info.nselected == 2000


def test_the_host_route_of_the_nfa_tier(gpu, monkeypatch):
    data = random_lines(5, 600)
    with S.Pool() as pool:
        p = Program(pool, DOTTED, S.ENGINE_NFA)
        _, one, _ = run_extract(p.sc, p.exp, data, [1, 0], src_off=3, dst_off=5)
        assert p.sc.last_lines_device == 1
        monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
        _, two, _ = run_extract(p.sc, p.exp, data, [1, 0], src_off=3, dst_off=5)
        assert p.sc.last_lines_device == 0 and one == two


# ------------------------------------------------------------------ 5. bad arguments

def test_bad_arguments(gpu):
    data = b"\n".join(URI_LINES)
    src = upload_at(data, 0)
    out = Out(gpu, 4096, 0)
    info = (ctypes.c_size_t * 5)()

    def call(sc, groups=(0,), ngroups=None, delim=0x0A, fsep=0x09, flags=0, out_ptr=None, cap=4096):
        arr = (ctypes.c_int * max(len(groups), 1))(*groups) if groups is not None else None
        n = (len(groups) if groups is not None else 1) if ngroups is None else ngroups
        return gpu.sre_hip_extract_lines(sc.h, src.ptr, len(data), delim, arr, n, fsep, flags,
                                         out.ptr if out_ptr is None else out_ptr, cap, None, 0, info, None)
    try:
        with S.Pool() as pool:
            re = S.parse(pool, URI)
            prog = S.compile(pool, re)
            sc = S.Scanner(pool, prog, FIRST)
            max_ncaps = (sc.slots - 2) // 2 - 1
            assert max_ncaps == 4
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                assert call(S.Scanner(pool, prog, mode)) == -1
            assert call(sc, groups=(), ngroups=0) == -1
            assert call(sc, groups=(0,) * 33) == -1
            assert call(sc, groups=None) == -1
            assert call(sc, groups=(max_ncaps + 1,)) == -1
            assert call(sc, groups=(1, -1)) == -1
            for flags in (S.HIP_LINES_INVERT, S.HIP_LINES_ALL | S.HIP_LINES_INVERT, 4, 4 | S.HIP_LINES_ALL):
                assert call(sc, flags=flags) == -1
            for bad in (-1, 256):
                assert call(sc, fsep=bad) == -1
                assert call(sc, delim=bad) == -1
            # the output inside, in front of and behind the source, overlapping it
            for o, cap in [(src.ptr + 5, 8), (src.ptr - 4, 5), (src.ptr + len(data) - 1, 64)]:
                assert call(sc, out_ptr=o, cap=cap) == -1
            with pytest.raises(RuntimeError):
                sc.extract_lines(src.ptr, len(data), [], out.ptr, 4096)
            out.check(b"")
            assert download(gpu, src.ptr, len(data)) == data
            # the limits themselves are fine
            assert call(sc, groups=(max_ncaps,) * 32) == 0
            assert S.HIP_EXTRACT_MAX_FIELDS == 32
    finally:
        src.free()
        out.free()


# ------------------------------------------------------------------ 6. truncation

WORDS = [b"ab@ab.ab", b"x", b"", b"  ", b"http://h.i/p?q", b"nothing here", b"1.2.3.4", b"f://g", b"10.20.30.40" * 3,
         b"zz://" + b"y" * 70 + b"/"]


def small_buffer(seed, nlines=120, lo=0, hi=6):
    rng = random.Random(seed)
    lines = [b" ".join(rng.choice(WORDS) for _ in range(rng.randrange(lo, hi))) for _ in range(nlines)]
    lines[-1] += b"end"                 # (an empty last line would be none: the buffer would end with the delimiter)
    return b"\n".join(lines)


def test_truncation(gpu):
    with S.Pool() as pool:
        p = Program(pool, URI)
        data = small_buffer(10)
        groups = [2, 0, 3]
        info, full, sel = run_extract(p.sc, p.exp, data, groups, src_off=1)
        need, first = info.need_bytes, len(row_text(data, sel[0][3], 0x09, 0x0A))
        assert len(sel) > 8 and first > 3
        for dst_off in (0, 5):
            for cap, nwritten in [(need, len(sel)), (need - 1, len(sel) - 1), (first, 1), (first - 1, 0), (need // 2, None)]:
                info, part, _ = run_extract(p.sc, p.exp, data, groups, src_off=1, dst_off=dst_off, out_cap=cap)
                assert info.need_bytes == need and info.nselected == len(sel)
                assert nwritten is None or info.nwritten == nwritten
                assert info.out_bytes <= cap and full.startswith(part) and (part == b"" or part.endswith(b"\n"))
        # a sizing call: no output buffer at all
        info, _, _ = run_extract(p.sc, p.exp, data, groups, out_cap=0, null_out=True, index_cap=0)
        assert info == S.FilterInfo(len(split_lines(data, 0x0A)), len(sel), need, 0, 0)
        # fewer index rows than written rows, and no index at all
        for icap in (0, 1, 5, len(sel) - 1):
            info, _, _ = run_extract(p.sc, p.exp, data, groups, index_cap=icap)
            assert info.nwritten == len(sel)
        info, _, _ = run_extract(p.sc, p.exp, data, groups, out_cap=need // 2, index_cap=3)
        assert 3 < info.nwritten < len(sel)


# ------------------------------------------------------------------ 7. every line

def test_all_lines(gpu):
    with S.Pool() as pool:
        p = Program(pool, URI)
        data = small_buffer(11)
        groups = [1, 4, 2]
        info, want, sel = run_extract(p.sc, p.exp, data, groups, all_lines=True, dst_off=9)
        assert info.nselected == info.nwritten == info.nlines == 120
        rows = want.split(b"\n")[:-1]
        assert len(rows) == 120
        missed = [i for i, _, _, f in sel if f == [None] * 3]
        assert 10 < len(missed) < 110
        nohit = {i for i, (st, n) in enumerate(split_lines(data, 0x0A)) if p.exp.record(data[st:st + n], FIRST)[0] == S.SRE_DECLINED}
        assert set(missed) == nohit                        # (groups 1 and 2 of a URI match are always set)
        assert all(rows[i] == b"\t\t" for i in missed)


# ------------------------------------------------------------------ 8. several batches

@pytest.mark.parametrize("pats,engine,groups", [(URI, S.ENGINE_AUTO, [1, 2, 0]), (DOTTED, S.ENGINE_NFA, [0, 1, 1]),
                                                (URI, S.ENGINE_VM, [2, 0, 4, 1])],
                         ids=["scan", "nfa", "vm"])
def test_several_batches(gpu, monkeypatch, pats, engine, groups):
    """(vm: the per-line host route, which uploads the entries of a batch at d_val + i0 * k and d_start + i0 * k)"""
    device = 0 if engine == S.ENGINE_VM else 1
    with S.Pool() as pool:
        p = Program(pool, pats, engine)
        assert engine == S.ENGINE_AUTO or p.sc.engine == engine
        data = small_buffer(12, nlines=100)
        assert len(split_lines(data, 0x0A)) == 100
        info, one, _ = run_extract(p.sc, p.exp, data, groups, src_off=2, dst_off=9)
        assert p.sc.last_line_batches == 1 and p.sc.last_lines_device == device and 0 < info.nselected < 100
        monkeypatch.setenv("SRE_HIP_LINES_BATCH", "7")
        for all_lines in (False, True):
            _, many, _ = run_extract(p.sc, p.exp, data, groups, src_off=2, dst_off=9, all_lines=all_lines)
            assert p.sc.last_line_batches == 15 and p.sc.last_lines_device == device
            assert all_lines or many == one


# ------------------------------------------------------------------ 9. entry blocks

def test_cuts_inside_entry_blocks(gpu):
    """2000 lines x 3 fields are 6000 entries, six workgroups of the scan; 1024 is no multiple of 3, so the line
    boundaries do not fall on the block boundaries.  Entry block b holds the lines 1024 b / 3 .. 1024 (b + 1) / 3"""
    with S.Pool() as pool:
        p = Program(pool, URI)
        data = small_buffer(13, nlines=2000, lo=1, hi=4)
        groups = [1, 0, 2]
        for all_lines in (True, False):
            sel = expected(p.exp, data, 0x0A, groups, all_lines)
            sizes = [len(row_text(data, f, 0x09, 0x0A)) for _, _, _, f in sel]
            assert all_lines or 700 < len(sel) < 1900
            for line in (400, 1024 // 3 + 1, 1500, 4096 // 3, 5 * 1024 // 3):      # inside the second and the fifth block
                k = sum(1 for i, _, _, _ in sel if i < line)                       # rows in front of that line
                for cap in (sum(sizes[:k]), sum(sizes[:k]) + sizes[k] - 1):
                    info, _, _ = run_extract(p.sc, p.exp, data, groups, src_off=1, dst_off=2, all_lines=all_lines, out_cap=cap)
                    assert info.nwritten == k and info.nselected == len(sel)


# ------------------------------------------------------------------ 10. against the filter

def test_whole_lines_equal_the_filter_output(gpu):
    data = random_lines(6)[:60000]
    lines = split_lines(data, 0x0A)
    want = b"".join(data[st:st + n] + b"\n" for st, n in lines)
    with S.Pool() as pool:
        re = S.parse(pool, [rb"(.*)"])
        prog = S.compile(pool, re)
        sc = S.Scanner(pool, prog, FIRST)
        src = upload_at(data, 7)
        a, b = Out(gpu, len(want) + 11, 1), Out(gpu, len(want) + 11, 1)
        try:
            fi = sc.filter_lines(src.ptr + 7, len(data), a.ptr, a.cap, all_lines=True)
            assert fi.out_bytes == len(want)
            a.check(want)
            for groups in ([1], [0]):
                info = sc.extract_lines(src.ptr + 7, len(data), groups, b.ptr, b.cap)
                assert info == fi
                b.check(want)
                assert download(gpu, b.buf.ptr, b.total) == download(gpu, a.buf.ptr, a.total)
        finally:
            src.free()
            a.free()
            b.free()


# ------------------------------------------------------------------ 11. coexistence

def test_other_calls_are_unchanged_by_an_extract_call(gpu):
    with S.Pool() as pool:
        for pats, engine in [(URI, S.ENGINE_AUTO), (DOTTED, S.ENGINE_NFA)]:
            p = Program(pool, pats, engine)
            sc = p.sc
            data = random_lines(7)[:40000]
            small = small_buffer(14, nlines=30)
            lines = split_lines(data, 0x0A)
            src = upload_at(data, 5)
            out = Out(gpu, 3 * len(data) + 3 * len(lines) + 1, 3)
            try:
                base = src.ptr + 5
                before = sc.scan_lines(base, len(data), cap=len(lines) + 1)
                diag = (sc.last_lines_device, sc.last_line_batches, sc.last_short_lines, sc.last_fixups)
                batched = sc.scan([base + st for st, _ in lines], [n for _, n in lines])
                filtered = sc.filter_lines(base, len(data), out.ptr, out.cap)
                text = download(gpu, out.ptr, filtered.out_bytes)
                info = sc.extract_lines(base, len(data), [0, 1, 0], out.ptr, out.cap)
                assert info.nselected == before[1] == filtered.nselected
                assert (sc.last_lines_device, sc.last_line_batches, sc.last_short_lines, sc.last_fixups) == diag
                with pytest.raises(RuntimeError):
                    sc.results()            # the extract call replaced the scanner's last call, as scan_lines does
                assert sc.scan_lines(base, len(data), cap=len(lines) + 1) == before
                # the filter after a (larger) extract call, and a small extract after a large filter: the shared arrays
                assert sc.filter_lines(base, len(data), out.ptr, out.cap) == filtered
                assert download(gpu, out.ptr, filtered.out_bytes) == text
                run_extract(sc, p.exp, small, [1, 0])
                assert sc.filter_lines(base, len(data), out.ptr, out.cap) == filtered
                assert download(gpu, out.ptr, filtered.out_bytes) == text
                run_extract(sc, p.exp, small, [0, 1, 1, 0], all_lines=True)
                assert sc.scan([base + st for st, _ in lines], [n for _, n in lines]) == batched
                assert sc.scan_lines(base, len(data), all_lines=True, cap=len(lines) + 1)[1] == len(lines)
            finally:
                src.free()
                out.free()
