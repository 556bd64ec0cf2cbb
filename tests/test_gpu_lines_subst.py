"""The line substitute (sre_hip_substitute_lines): every matching line of a device buffer with its first match
replaced by a template, as rows in another device buffer, with an optional device-side index.

Expected output is pure Python: the split rule of line mode, the oracle's first-match record of every line, slicing,
and the template applied piece by piece as sregex_amd.template_pieces lists them.  Every output buffer has 64 guard
bytes in front and behind and is pre-filled with 0xA5 (the filter test's Out); every check asserts that the guards and
everything at or beyond out_bytes still hold 0xA5.
"""
import ctypes
import random
import re

import pytest

import sregex_amd as S
from test_gpu_lines import split_lines, upload_at
from test_gpu_lines_filter import Out, download
from test_gpu_lines_extract import (BRACKET, DOTTED, EMPTY_MATCH_LINES, HEADLINE, LENGTHS, ROUTES, URI, URI_LINES, Program,
                                    bracketed_buffer, random_lines, small_buffer)
from test_gpu_nfa_wide import WIDE

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
WIDTH = 8


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def max_group(sc):
    return (sc.slots - 2) // 2 - 1


def pieces_of(template, mg):
    """the template as a list of pieces, bytes (a literal) or an int (a group); their kinds are template_pieces'"""
    out = []
    for m in re.finditer(rb"\$\$|\$\{(\d+)\}|\$(\d+)|[^$]+", template, re.S):
        if m.group(1) is not None or m.group(2) is not None:
            out.append(int(m.group(1) or m.group(2)))
        else:
            lit = b"$" if m.group(0) == b"$$" else m.group(0)
            if out and isinstance(out[-1], bytes):
                out[-1] += lit
            else:
                out.append(lit)
    assert [p if isinstance(p, int) else -1 for p in out] == S.template_pieces(template, mg), template
    return out


def expected(exp, data, delim, pieces, all_lines):
    """[(line, start, len, (match offset in the buffer, match length, replacement length) or None, row text)] of the
    selected lines"""
    out = []
    for i, (st, n) in enumerate(split_lines(data, delim)):
        line = data[st:st + n]
        rec = exp.record(line, FIRST)
        hit = rec[0] != S.SRE_DECLINED
        if not (hit or all_lines):
            continue
        if not hit:
            out.append((i, st, n, None, line))
            continue
        m0, m1 = rec[2], rec[3]
        assert 0 <= m0 <= m1 <= n
        repl = b""
        for p in pieces:
            if isinstance(p, bytes):
                repl += p
            else:
                a, b = rec[2 + 2 * p], rec[3 + 2 * p]
                repl += line[a:b] if 0 <= a <= b <= n else b""
        out.append((i, st, n, (st + m0, m1 - m0, len(repl)), line[:m0] + repl + line[m1:]))
    return out


def run_subst(sc, exp, data, template, delim=0x0A, src_off=0, dst_off=0, all_lines=False, out_cap=None, index_cap=None,
              null_out=False):
    """one call, checked in full: info, output, guards, index rows; returns (info, output bytes, expected rows)"""
    lib = sc.lib
    d = bytes([delim])
    sel = expected(exp, data, delim, pieces_of(template, max_group(sc)), all_lines)
    texts = [row + d for _, _, _, _, row in sel]
    need = sum(len(t) for t in texts)
    assert need == sum(n - (m[1] if m else 0) + (m[2] if m else 0) + 1 for _, _, n, m, _ in sel)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for t in texts:
        if out_bytes + len(t) > cap:
            break
        out_bytes += len(t)
        nwritten += 1
    want = b"".join(texts[:nwritten])
    icap = len(sel) + 3 if index_cap is None else index_cap
    src = upload_at(data, src_off)
    out = Out(lib, cap, dst_off)
    idx = Out(lib, icap * WIDTH * 8, 0)
    try:
        info = sc.substitute_lines(src.ptr + src_off, len(data), template, None if null_out else out.ptr, cap, delim, all_lines,
                                   idx.ptr if icap else None, icap)
        assert info == S.FilterInfo(len(split_lines(data, delim)), len(sel), need, nwritten, out_bytes), (info, len(sel), need)
        out.check(want)
        assert download(lib, src.ptr + src_off, len(data)) == data
        nrows = min(icap, nwritten)
        rows, o = [], 0
        for (i, st, n, m, _), t in zip(sel[:nrows], texts):
            rows.append((i, st, n, o, m[0], m[1], o + (m[0] - st), m[2]) if m else (i, st, n, o, -1, -1, -1, -1))
            o += len(t)
        raw = (ctypes.c_int64 * (WIDTH * nrows)).from_buffer_copy(download(lib, idx.ptr, 8 * WIDTH * nrows)) if nrows else []
        got = [tuple(raw[WIDTH * r:WIDTH * (r + 1)]) for r in range(nrows)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
        idx.check(download(lib, idx.ptr, 8 * WIDTH * nrows))      # nothing behind the rows, nothing around the index
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
                for template in (b"", b"<$0>", b"$0"):
                    for data in [b"", d, b"a" + d + d + b"b", b"a", d * 5, d * 40 + b"a"]:
                        for all_lines in (False, True):
                            info, _, _ = run_subst(p.sc, p.exp, data, template, delim, all_lines=all_lines)
                        if data == b"":
                            assert info == S.FilterInfo(0, 0, 0, 0, 0)
                        assert info.nselected == info.nlines


@pytest.mark.parametrize("delim", [0x0A, ord("a")], ids=["newline", "a"])
def test_an_empty_match_at_either_end_of_the_line(gpu, delim):
    """sed 's/^/> /' and sed 's/$/;/': the empty match at offset 0 of a line that is not empty, and at its end.  With
    the delimiter "a" the byte behind a line's end (and the one in front of its start) is a word character, and the line
    is still its own stream: \\b in front of "b cd" and $ behind it match"""
    d = bytes([delim])
    data = d.join(EMPTY_MATCH_LINES)
    lines = [data[st:st + n] for st, n in split_lines(data, delim)]
    assert sum(1 for line in lines if line) >= 5 and b"" in lines
    with S.Pool() as pool:
        for pat, template, row in [(rb"^", b"> ", lambda line: b"> " + line), (rb"$", b";", lambda line: line + b";"),
                                   (rb"^", b"", lambda line: line), (rb"\b", b"> ", None), (rb"\b", b";", None)]:
            p = Program(pool, [pat], key=False)
            for all_lines in (False, True):
                _, want, sel = run_subst(p.sc, p.exp, data, template, delim, src_off=1, dst_off=3, all_lines=all_lines)
                if row:
                    assert len(sel) == len(lines) and want == b"".join(row(line) + d for line in lines)
                elif not all_lines:
                    # a line with a word character gets the template in front of its first word
                    words = [line for line in lines if any(bytes([c]).isalnum() for c in line)]
                    assert [r for _, _, _, _, r in sel] == [w[:len(w) - len(w.lstrip())] + template + w.lstrip() for w in words]
                    assert any(w[:1] != b" " for w in words) and any(w[:1] == b" " for w in words)


# ------------------------------------------------------------------ 2. identity

NEVER = [rb"QQZ(Q)"]


@pytest.mark.parametrize("pats,engine,template", [(HEADLINE, S.ENGINE_AUTO, b"$0"), (URI, S.ENGINE_AUTO, b"$0"),
                                                  (DOTTED, S.ENGINE_NFA, b"$0"), (NEVER, S.ENGINE_AUTO, b"<$1>$0-"),
                                                  (NEVER, S.ENGINE_AUTO, b"")],
                         ids=["headline", "uri", "dotted-nfa", "no-match", "no-match-delete"])
def test_the_match_for_the_match_is_the_filter_output(gpu, pats, engine, template):
    data = random_lines(6)[:60000]
    want = b"".join(data[st:st + n] + b"\n" for st, n in split_lines(data, 0x0A))
    with S.Pool() as pool:
        sc = S.Scanner(pool, S.compile(pool, S.parse(pool, pats)), FIRST, engine)
        assert engine == S.ENGINE_AUTO or sc.engine == engine
        src = upload_at(data, 7)
        a, b = Out(gpu, len(want) + 11, 1), Out(gpu, len(want) + 11, 1)
        try:
            fi = sc.filter_lines(src.ptr + 7, len(data), a.ptr, a.cap, all_lines=True)
            assert fi.out_bytes == len(want)
            a.check(want)
            info = sc.substitute_lines(src.ptr + 7, len(data), template, b.ptr, b.cap, all_lines=True)
            assert info == fi
            b.check(want)
            assert download(gpu, b.buf.ptr, b.total) == download(gpu, a.buf.ptr, a.total)
            if pats is NEVER:
                assert sc.substitute_lines(src.ptr + 7, len(data), template, b.ptr, b.cap) == S.FilterInfo(fi.nlines, 0, 0, 0, 0)
                b.check(want)           # (nothing written: what the call before left)
        finally:
            src.free()
            a.free()
            b.free()


# ------------------------------------------------------------------ 3. alignment and lengths

LITERAL33 = b"0123456789abcdefghijklmnopqrstuvw"


@pytest.mark.parametrize("template", [b"($1)", b"", b"$1$1", LITERAL33 + b"$0"], ids=["paren", "delete", "twice", "literal33"])
def test_alignment_and_lengths(gpu, template):
    assert len(LITERAL33) == 33
    rng = random.Random(51)
    # the extract test's buffer, and one line of 200 KiB with its match in the middle: the text in front of the match
    # and the text behind it span many tiles each
    data = bracketed_buffer(rng) + b"\n" + b"x" * (100 * 1024) + b"[mid]" + b"y" * (100 * 1024) + b"\nlast [] line"
    with S.Pool() as pool:
        p = Program(pool, BRACKET)
        for src_off in (0, 1, 7, 15):
            for dst_off in (0, 1, 8, 15):
                info, _, sel = run_subst(p.sc, p.exp, data, template, src_off=src_off, dst_off=dst_off)
                assert info.nselected == len(LENGTHS) + 3 == info.nlines - 1
        run_subst(p.sc, p.exp, data, template, src_off=3, dst_off=5, all_lines=True)
        assert sorted(m[1] - 2 for _, _, _, m, _ in sel) == sorted(LENGTHS + [200 * 1024, 3, 0])


# ------------------------------------------------------------------ 4. literal alignments

@pytest.mark.parametrize("L", [1, 15, 16, 17, 33])
def test_literal_alignments(gpu, L):
    data = b"\n".join(URI_LINES * 3)
    lit = bytes(0x41 + (x * 5) % 26 for x in range(L))
    with S.Pool() as pool:
        p = Program(pool, URI)
        for r in range(17):
            info, _, _ = run_subst(p.sc, p.exp, data, b"x" * r + b"$1" + lit, src_off=r % 16, dst_off=(3 * r) % 16,
                                   all_lines=bool(r & 1))
            assert 0 < info.nselected <= info.nlines


# ------------------------------------------------------------------ 5. tiny rows, many entries

def test_tiny_rows_of_many_entries(gpu):
    """3000 lines x 5 entries are 15000 entries, fifteen workgroups of the scan; a row has 2 bytes, so a tile of the
    gather meets thousands of entries, most of them empty.  Entry block b holds the lines 1024 b / 5 .. 1024 (b + 1) / 5"""
    with S.Pool() as pool:
        p = Program(pool, [rb"k=(\d)(x)?(y)?"], key=False)
        for data, all_lines in [(b"\n".join([b"k=1"] * 3000), False),
                                (b"\n".join(b"k=z" if i % 3 == 1 else b"k=1" for i in range(3000)), True),
                                (b"\n".join(b"k=z" if i % 3 == 1 else b"k=1" for i in range(3000)), False)]:
            info, want, sel = run_subst(p.sc, p.exp, data, b"$2$1$3", src_off=1, dst_off=2, all_lines=all_lines)
            assert info.nselected == info.nwritten == (3000 if all_lines or b"z" not in data else 2000)
            assert want.startswith(b"1\nk=z\n1\n" if all_lines else b"1\n1\n")
            sizes = [len(row) + 1 for _, _, _, _, row in sel]
            for line in (1024 // 5 + 1, 300, 2047 // 5, 4096 // 5 + 1, 900, 5119 // 5):     # inside the second and the fifth block
                k = sum(1 for i, _, _, _, _ in sel if i < line)                             # rows in front of that line
                for cap in (sum(sizes[:k]), sum(sizes[:k]) + sizes[k] - 1):
                    info, part, _ = run_subst(p.sc, p.exp, data, b"$2$1$3", src_off=1, dst_off=2, all_lines=all_lines, out_cap=cap,
                                              index_cap=4)
                    assert info.nwritten == k and info.nselected == len(sel)
                    assert part == want[:info.out_bytes] and part.endswith(b"\n")


# ------------------------------------------------------------------ 6. unset against empty, several regexes

def test_unset_against_empty_and_several_regexes(gpu):
    with S.Pool() as pool:
        q = Program(pool, [rb"x(a*)y|z(b)?"])
        data = b"\n".join([b"xy", b"xaay", b"z", b"zb", b"w", b"--xy--", b"xaaaaaaaaaaaaaaaaay z"])
        _, want, _ = run_subst(q.sc, q.exp, data, b"[$1|$2]")
        assert want == b"[|]\n[aa|]\n[|]\n[|b]\n--[|]--\n[aaaaaaaaaaaaaaaaa|] z\n"
        _, want, _ = run_subst(q.sc, q.exp, data, b"[$1|$2]", all_lines=True, dst_off=3)
        assert want == b"[|]\n[aa|]\n[|]\n[|b]\nw\n--[|]--\n[aaaaaaaaaaaaaaaaa|] z\n"
        # several regexes: the groups are those of the regex that matched
        m = Program(pool, [rb"k=(\d+)", rb"([a-z]+)@([a-z]+)"])
        data = b"\n".join([b"k=12 ab@cd", b"ab@cd k=12", b"none", b"k=", b"zz@y"])
        _, want, _ = run_subst(m.sc, m.exp, data, b"<$1,$2>")
        assert want == b"<12,> ab@cd\n<ab,cd> k=12\n<zz,y>\n"
        _, want, _ = run_subst(m.sc, m.exp, data, b"<$1,$2>", all_lines=True)
        assert want == b"<12,> ab@cd\n<ab,cd> k=12\nnone\nk=\n<zz,y>\n"


# ------------------------------------------------------------------ 7. every route

def every_group(ncaps):
    t = b"<" + b"".join(b"${%d}" % g for g in range(ncaps + 1)) + b">"
    assert ncaps + 3 <= S.HIP_SUBST_MAX_PIECES
    return t


@pytest.mark.parametrize("name,pats,engine,routed,device", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route(gpu, name, pats, engine, routed, device):
    # (test_gpu_lines_extract.py asserts on the same buffer and programs that some and not all of the 2000 lines match)
    data = random_lines(5)
    with S.Pool() as pool:
        p = Program(pool, pats, engine)
        assert p.sc.engine == routed
        if name.startswith("nfa-wide"):
            assert p.sc.nfa_bits == WIDE[1][1]
        template = every_group(p.ncaps)
        info, _, _ = run_subst(p.sc, p.exp, data, template, src_off=3, dst_off=5)
        assert p.sc.last_lines_device == device and p.sc.last_line_batches >= 1
        assert 0 < info.nselected < info.nlines == 2000, info
        info, _, _ = run_subst(p.sc, p.exp, data, template, src_off=3, dst_off=5, all_lines=True)
        assert p.sc.last_lines_device == device
        assert info.nselected == 2000


def test_the_host_route_of_the_nfa_tier(gpu, monkeypatch):
    data = random_lines(5, 600)
    with S.Pool() as pool:
        p = Program(pool, DOTTED, S.ENGINE_NFA)
        for all_lines in (False, True):
            monkeypatch.delenv("SRE_HIP_LINES_NFA_HOST", raising=False)
            _, one, _ = run_subst(p.sc, p.exp, data, b"[$1$0]", src_off=3, dst_off=5, all_lines=all_lines)
            assert p.sc.last_lines_device == 1
            monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
            _, two, _ = run_subst(p.sc, p.exp, data, b"[$1$0]", src_off=3, dst_off=5, all_lines=all_lines)
            assert p.sc.last_lines_device == 0 and one == two


# ------------------------------------------------------------------ 8. truncation

def test_truncation(gpu):
    with S.Pool() as pool:
        p = Program(pool, URI)
        data = small_buffer(10)
        template = b"$2|$0|$3"
        info, full, sel = run_subst(p.sc, p.exp, data, template, src_off=1)
        need, first = info.need_bytes, len(sel[0][4]) + 1
        assert len(sel) > 8 and first > 3
        for dst_off in (0, 5):
            for cap, nwritten in [(need, len(sel)), (need - 1, len(sel) - 1), (first, 1), (first - 1, 0), (need // 2, None)]:
                info, part, _ = run_subst(p.sc, p.exp, data, template, src_off=1, dst_off=dst_off, out_cap=cap)
                assert info.need_bytes == need and info.nselected == len(sel)
                assert nwritten is None or info.nwritten == nwritten
                assert info.out_bytes <= cap and full.startswith(part) and (part == b"" or part.endswith(b"\n"))
        # a sizing call: no output buffer at all
        info, _, _ = run_subst(p.sc, p.exp, data, template, out_cap=0, null_out=True, index_cap=0)
        assert info == S.FilterInfo(len(split_lines(data, 0x0A)), len(sel), need, 0, 0)
        # fewer index rows than written rows, and no index at all
        for icap in (0, 1, 5, len(sel) - 1):
            info, _, _ = run_subst(p.sc, p.exp, data, template, index_cap=icap)
            assert info.nwritten == len(sel)
        info, _, _ = run_subst(p.sc, p.exp, data, template, out_cap=need // 2, index_cap=3, all_lines=True)
        assert 3 < info.nwritten < 120


# ------------------------------------------------------------------ 9. several batches

@pytest.mark.parametrize("pats,engine,template", [(URI, S.ENGINE_AUTO, b"$1:$2"), (DOTTED, S.ENGINE_NFA, b"<$0$1>"),
                                                  (URI, S.ENGINE_VM, b"$2 $4|$1")],
                         ids=["scan", "nfa", "vm"])
def test_several_batches(gpu, monkeypatch, pats, engine, template):
    """(vm: the per-line host route, which uploads the entries of a batch at d_val + i0 * P and d_start + i0 * P)"""
    device = 0 if engine == S.ENGINE_VM else 1
    with S.Pool() as pool:
        p = Program(pool, pats, engine)
        assert engine == S.ENGINE_AUTO or p.sc.engine == engine
        data = small_buffer(12, nlines=100)
        assert len(split_lines(data, 0x0A)) == 100
        info, one, _ = run_subst(p.sc, p.exp, data, template, src_off=2, dst_off=9)
        _, one_all, _ = run_subst(p.sc, p.exp, data, template, src_off=2, dst_off=9, all_lines=True)
        assert p.sc.last_line_batches == 1 and p.sc.last_lines_device == device and 0 < info.nselected < 100
        monkeypatch.setenv("SRE_HIP_LINES_BATCH", "7")
        for all_lines in (False, True):
            _, many, _ = run_subst(p.sc, p.exp, data, template, src_off=2, dst_off=9, all_lines=all_lines)
            assert p.sc.last_line_batches == 15 and p.sc.last_lines_device == device
            assert many == (one_all if all_lines else one)


# ------------------------------------------------------------------ 10. bad arguments

def test_bad_arguments(gpu):
    data = b"\n".join(URI_LINES)
    src = upload_at(data, 0)
    out = Out(gpu, 65536, 0)
    info = (ctypes.c_size_t * 5)()

    def call(sc, template=b"<$1>", delim=0x0A, flags=0, out_ptr=None, cap=65536):
        return gpu.sre_hip_substitute_lines(sc.h, src.ptr, len(data), delim, template, len(template), flags,
                                            out.ptr if out_ptr is None else out_ptr, cap, None, 0, info, None)
    try:
        with S.Pool() as pool:
            re_ = S.parse(pool, URI)
            prog = S.compile(pool, re_)
            sc = S.Scanner(pool, prog, FIRST)
            assert max_group(sc) == 4
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                assert call(S.Scanner(pool, prog, mode)) == -1
            for bad in (b"$", b"$x", b"${1", b"${}", b"x$", b"$1x" * 15 + b"$1", b"y" * 4097):
                assert call(sc, bad) == -1, bad
            assert call(sc, b"a\nb") == -1                      # a literal delimiter
            assert call(sc, b"a$$b", delim=ord("$")) == -1
            assert call(sc, b"a\x00b", delim=0) == -1
            assert call(sc, b"$5") == -1 and call(sc, b"${5}") == -1 and call(sc, b"$10") == -1
            for flags in (S.HIP_LINES_INVERT, S.HIP_LINES_ALL | S.HIP_LINES_INVERT, 4):
                assert call(sc, flags=flags) == -1
            for bad in (-1, 256):
                assert call(sc, delim=bad) == -1
            # the output inside, in front of and behind the source, overlapping it
            for o, cap in [(src.ptr + 5, 8), (src.ptr - 4, 5), (src.ptr + len(data) - 1, 64)]:
                assert call(sc, out_ptr=o, cap=cap) == -1
            with pytest.raises(RuntimeError):
                sc.substitute_lines(src.ptr, len(data), b"$9", out.ptr, 4096)
            out.check(b"")
            assert download(gpu, src.ptr, len(data)) == data
            # the limits themselves are fine
            assert call(sc, b"$4x" * 15) == 0 and info[1] > 0
            assert call(sc, b"y" * 4096) == 0 and info[2] > 4096 * info[1]
            assert call(sc, b"a\x00b") == 0
    finally:
        src.free()
        out.free()


# ------------------------------------------------------------------ 11. coexistence

def test_other_calls_are_unchanged_by_a_substitute_call(gpu):
    with S.Pool() as pool:
        for pats, engine in [(URI, S.ENGINE_AUTO), (DOTTED, S.ENGINE_NFA)]:
            p = Program(pool, pats, engine)
            sc = p.sc
            data = random_lines(7)[:40000]
            small = small_buffer(14, nlines=30)
            lines = split_lines(data, 0x0A)
            src = upload_at(data, 5)
            out = Out(gpu, 3 * len(data) + 40 * len(lines) + 1, 3)
            try:
                base = src.ptr + 5
                before = sc.scan_lines(base, len(data), cap=len(lines) + 1)
                diag = (sc.last_lines_device, sc.last_line_batches, sc.last_short_lines, sc.last_fixups)
                batched = sc.scan([base + st for st, _ in lines], [n for _, n in lines])
                filtered = sc.filter_lines(base, len(data), out.ptr, out.cap)
                text = download(gpu, out.ptr, filtered.out_bytes)
                extracted = sc.extract_lines(base, len(data), [1, 0], out.ptr, out.cap)
                fields = download(gpu, out.ptr, extracted.out_bytes)
                info = sc.substitute_lines(base, len(data), b"<$1-$0-$1>" + LITERAL33, out.ptr, out.cap)
                assert info.nselected == before[1] == filtered.nselected == info.nwritten
                assert (sc.last_lines_device, sc.last_line_batches, sc.last_short_lines, sc.last_fixups) == diag
                with pytest.raises(RuntimeError):
                    sc.results()            # the call replaced the scanner's last call, as scan_lines does
                assert sc.scan_lines(base, len(data), cap=len(lines) + 1) == before
                # large then small and small then large across the three calls: the shared arrays, the literal block
                assert sc.filter_lines(base, len(data), out.ptr, out.cap) == filtered
                assert download(gpu, out.ptr, filtered.out_bytes) == text
                run_subst(sc, p.exp, small, b"$1")
                assert sc.extract_lines(base, len(data), [1, 0], out.ptr, out.cap) == extracted
                assert download(gpu, out.ptr, extracted.out_bytes) == fields
                run_subst(sc, p.exp, small, b"ab$0" + b"c" * 40, all_lines=True)
                assert sc.filter_lines(base, len(data), out.ptr, out.cap) == filtered
                assert download(gpu, out.ptr, filtered.out_bytes) == text
                sc.extract_lines(base, 9, [0], out.ptr, out.cap)
                run_subst(sc, p.exp, data, b"ab$0" + b"c" * 40)         # the same literals: nothing uploaded
                run_subst(sc, p.exp, data, b"$1" + b"d" * 40 + b"$0", all_lines=True)
                assert sc.scan([base + st for st, _ in lines], [n for _, n in lines]) == batched
                assert sc.scan_lines(base, len(data), all_lines=True, cap=len(lines) + 1)[1] == len(lines)
            finally:
                src.free()
                out.free()
