"""The gather of the line extract (sre_hip_extract_lines) on the CPU: tests/lines_extract_sim.cpp walks every output
chunk with the chunk logic the kernel compiles (sregex_amd/csrc/sre_lines_gather.h) over the entry table, tile by
tile with the kernel's table slices and LDS window rule, and counts every source byte read and every output byte
written.  A case is a list of lines and, per line, None (no match) or K spans (a, b) relative to the line (None: an
unset group); expected output is Python slicing."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32 = ctypes.c_uint64, ctypes.c_uint32
_p64, _p32, _p8 = ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_uint8)
_i64 = ctypes.c_int64
_pi64 = ctypes.POINTER(_i64)
FILL = 0xA5


@pytest.fixture(scope="module")
def esim():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "liblinesextractsim.so")
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, "lines_extract_sim.cpp"), os.path.join(csrc, "sre_lines_gather.h"),
            os.path.join(csrc, "sre_lines_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    L = ctypes.CDLL(so)
    L.lesim_window.restype = _u32
    for f in (L.lesim_flag_last, L.lesim_flag_unset, L.lesim_flag_first):
        f.restype = _u64
    L.lesim_cut.restype = _u64
    L.lesim_cut.argtypes = [_p64, _u64, _u64, _u64]
    L.lesim_gather.restype = _u64
    L.lesim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32,
                               _p64, _p64]
    L.lesim_select.restype = None
    L.lesim_select.argtypes = [_pi64, _u32, _u64, _i64, ctypes.c_int, _p64, _p64, _p32, _u32, _p64, _p64]
    return L


def entry_table(esim, lines, spans, K, all_lines):
    """(buffer, val, starts, rows): the per-entry values and start words as the select pass leaves them, and the
    expected row of every selected line"""
    LAST, UNSET, FIRST = esim.lesim_flag_last(), esim.lesim_flag_unset(), esim.lesim_flag_first()
    val, starts, rows, pos = [], [], [], 0
    for ln, sp in zip(lines, spans):
        assert sp is None or len(sp) == K
        selected = sp is not None or all_lines
        fields = []
        for f in range(K):
            s = sp[f] if sp is not None else None
            flags = (FIRST if f == 0 else 0) | (LAST if f == K - 1 else 0)
            if s is None:
                starts.append(pos | UNSET | flags)
                n = 0
                fields.append(b"")
            else:
                a, b = s
                assert 0 <= a <= b <= len(ln)
                starts.append((pos + a) | flags)
                n = b - a
                fields.append(ln[a:b])
            val.append(n + 1 if selected else 0)
        if selected:
            rows.append(fields)
        pos += len(ln) + 1
    return val, starts, rows


def run(esim, lines, spans, K, src_off, dst_off, all_lines=False, caps=(None,), delim=0x0A, fsep=0x09):
    """the model over one table for every out_cap of `caps` (None: everything fits; a callable gets (need, row
    sizes)); asserts the cut, where it reads and writes and what it writes; returns (windowed, global) of the last"""
    d, s = bytes([delim]), bytes([fsep])
    assert not any(d in ln for ln in lines)
    buf = d.join(lines) + d
    n = len(lines)
    val, starts, rows = entry_table(esim, lines, spans, K, all_lines)
    off = [0]
    for v in val:
        off.append(off[-1] + v)
    nent = n * K
    need = off[-1]
    texts = [s.join(r) + d for r in rows]
    assert sum(len(t) for t in texts) == need
    a_off, a_starts = (_u64 * (nent + 1))(*off), (_u64 * max(nent, 1))(*starts)
    src_len = (src_off + len(buf) + 15) // 16 * 16
    src = bytes([0xEE]) * src_off + buf + bytes([0xEE]) * (src_len - src_off - len(buf))
    res = None
    for cap in caps:
        cap = need if cap is None else cap(need, [len(t) for t in texts]) if callable(cap) else cap
        if cap < 0:
            continue
        want, k = b"", 0
        for t in texts:
            if len(want) + len(t) > cap:
                break
            want += t
            k += 1
        # the cut is made at a line boundary and counts whole rows
        i = esim.lesim_cut(a_off, n, K, cap)
        out_bytes = off[i * K]
        assert out_bytes == len(want) <= cap, (cap, i, out_bytes, len(want))
        assert sum(1 for e in range(0, i * K, K) if val[e]) == k
        assert all(val[e] for e in range(i * K)) or not all_lines
        dst_len = (dst_off + out_bytes + 15) // 16 * 16
        dst = (ctypes.c_uint8 * max(dst_len, 1))(*([FILL] * max(dst_len, 1)))
        reads = (_u32 * max(src_len, 1))()
        writes = (_u32 * max(dst_len, 1))()
        win, glo = _u64(), _u64()
        bad = esim.lesim_gather(a_off, a_starts, nent, out_bytes, src_off, dst_off, delim, fsep, src, src_len, dst, dst_len,
                                reads, writes, ctypes.byref(win), ctypes.byref(glo))
        ctx = (n, K, src_off, dst_off, cap, out_bytes)
        assert bad == 0, ("accesses outside the aligned extents", bad, ctx)
        got = bytes(dst)[:dst_len]
        if got[dst_off:dst_off + out_bytes] != want:
            g = got[dst_off:dst_off + out_bytes]
            at = next(x for x in range(out_bytes) if g[x] != want[x])
            raise AssertionError(("first difference at", at, g[max(0, at - 8):at + 8], want[max(0, at - 8):at + 8], ctx))
        w = list(writes)[:dst_len]
        assert w[dst_off:dst_off + out_bytes] == [1] * out_bytes, ("every output byte exactly once", ctx)
        assert not any(w[:dst_off]) and not any(w[dst_off + out_bytes:]), ("a write outside [out, out + out_bytes)", ctx)
        assert got[:dst_off] == bytes([FILL]) * dst_off and got[dst_off + out_bytes:] == bytes([FILL]) * (dst_len - dst_off - out_bytes)
        res = (win.value, glo.value)
    return res


# need, need - 1, one row, one row - 1, 0
CAPS = (None, lambda need, rows: need - 1, lambda need, rows: rows[0] if rows else 0,
        lambda need, rows: rows[0] - 1 if rows else 0, 0)


def text(rng, n):
    return bytes(rng.choice(b"abcdefgh@. \t") for _ in range(n))


def line_with_fields(rng, lens):
    """a line that holds one span per length of `lens` in order, with filler between; returns (line, spans)"""
    line, spans = b"", []
    for n in lens:
        line += text(rng, rng.randrange(0, 4))
        spans.append((len(line), len(line) + n))
        line += text(rng, n)
    return line + text(rng, rng.randrange(0, 4)), spans


LENS = [0, 1, 15, 16, 17, 31, 32, 33]


@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_field_lengths_and_cuts(esim, K):
    rng = random.Random(40 + K)
    lines, spans = [], []
    pool = LENS * K
    rng.shuffle(pool)
    for r in range(len(LENS)):
        ln, sp = line_with_fields(rng, pool[r * K:(r + 1) * K])
        lines.append(ln)
        spans.append(sp)
        if r % 3 == 1:
            lines.append(text(rng, 20))         # a line without a match
            spans.append(None)
    for so, do in [(0, 0), (1, 0), (0, 1), (7, 9), (15, 15), (3, 8)]:
        for all_lines in (False, True):
            run(esim, lines, spans, K, so, do, all_lines, CAPS)


def test_a_field_of_40_kib_and_its_neighbours(esim):
    rng = random.Random(41)
    big, sp = line_with_fields(rng, [3, 40 * 1024, 0])
    lines = [text(rng, 9), big, b"", text(rng, 40)]
    spans = [[(1, 4), None, (0, 9)], sp, None, [(0, 40), (40, 40), (39, 40)]]
    for so, do in [(0, 0), (5, 11), (15, 1)]:
        run(esim, lines, spans, 3, so, do, False, CAPS)
        run(esim, lines, spans, 3, so, do, True, CAPS)


def test_nested_overlapping_and_repeated_fields(esim):
    rng = random.Random(42)
    lines, spans = [], []
    for _ in range(60):
        ln = text(rng, rng.randrange(1, 70))
        a = rng.randrange(0, len(ln))
        b = rng.randrange(a, len(ln) + 1)
        c = rng.randrange(a, b + 1)
        # the whole match, a group inside it, the same group again, one that overlaps both, the whole line
        lines.append(ln)
        spans.append([(a, b), (c, b), (c, b), (a, c), (0, len(ln))])
    run(esim, lines, spans, 5, 3, 6, False, CAPS)
    run(esim, lines, [sp[:2] for sp in spans], 2, 9, 2, False, CAPS)


def test_empty_and_unset_runs_take_the_window_or_the_global_table(esim):
    rng = random.Random(43)
    W = esim.lesim_window()
    # more than W empty entries inside one tile: every entry takes one byte, the tile holds 16 Ki of them
    for K in (1, 3, 5):
        nl = (3 * W) // K + 7
        lines = [b"xy"] * nl
        spans = [[(1, 1) if (i + f) % 2 else None for f in range(K)] for i in range(nl)]
        win, glo = run(esim, lines, spans, K, 3, 5, False, (None, lambda need, rows: need - 1))
        assert glo >= 1, (K, win, glo)
    # fewer: the window
    lines = [b"xy"] * 100
    win, glo = run(esim, lines, [[None, (0, 0), (2, 2)]] * 100, 3, 1, 2)
    assert (win, glo) == (1, 0)
    # exactly the window and one entry more (K = 1: an entry per line)
    for cnt in (W, W + 1):
        win, glo = run(esim, [b""] * cnt, [[(0, 0)]] * cnt, 1, 0, 0)
        assert (win, glo) == ((1, 0) if cnt == W else (0, 1)), (cnt, win, glo)
    # a run of unselected lines (no entry of theirs takes a byte) between two rows, inside one tile
    lines = [text(rng, 30)] + [b"x"] * W + [text(rng, 30)]
    spans = [[(0, 30), (3, 9)]] + [None] * W + [[(2, 2), (0, 30)]]
    win, glo = run(esim, lines, spans, 2, 5, 1)
    assert (win, glo) == (0, 1)
    # ... and with ALL they give rows of two bytes: 2 W + 4 entries in the one tile, still beyond the window
    win, glo = run(esim, lines, spans, 2, 5, 1, all_lines=True)
    assert (win, glo) == (0, 1)


def test_every_alignment_pair(esim):
    rng = random.Random(44)
    lines, spans = [], []
    for n in (0, 1, 5, 16, 17, 33, 2, 47):
        ln, sp = line_with_fields(rng, [n, rng.randrange(0, 4)])
        lines.append(ln)
        spans.append(sp if n != 2 else None)
    spans[3] = [spans[3][0], None]
    for so in range(16):
        for do in range(16):
            run(esim, lines, spans, 2, so, do, bool((so + do) & 1), (None, lambda need, rows: need // 2))


def test_separator_equal_to_the_delimiter_and_other_bytes(esim):
    rng = random.Random(45)
    lines, spans = [], []
    for _ in range(40):
        ln, sp = line_with_fields(rng, [rng.randrange(0, 20) for _ in range(3)])
        lines.append(ln.replace(b"\n", b"?").replace(b"\x00", b"?"))
        spans.append(sp if rng.random() < 0.7 else None)
    for delim, fsep in [(0x0A, 0x0A), (0, 0), (0x0A, 0), (0, 255), (0x0A, ord(","))]:
        for all_lines in (False, True):
            run(esim, lines, spans, 3, 4, 13, all_lines, CAPS, delim=delim, fsep=fsep)


def test_random_tables(esim):
    rng = random.Random(int(os.environ.get("SRE_FUZZ_SEED", "20261017")) + 29)
    for k in range(60):
        K = rng.choice([1, 2, 3, 5])
        nlines = rng.choice([1, 2, 3, 10, 60]) if k % 15 else rng.choice([300, 1200])
        p = rng.choice([0.0, 0.1, 0.5, 0.9, 1.0])
        lines, spans = [], []
        for _ in range(nlines):
            ln = text(rng, rng.choice([0, 1, 15, 16, 17, 40, 90, 300]))
            sp = []
            for _ in range(K):
                if rng.random() < 0.2:
                    sp.append(None)
                else:
                    a = rng.randrange(0, len(ln) + 1)
                    sp.append((a, rng.randrange(a, len(ln) + 1)))
            lines.append(ln.replace(b"\n", b"?"))
            spans.append(sp if rng.random() < p else None)
        run(esim, lines, spans, K, rng.randrange(16), rng.randrange(16), bool(k & 1),
            (None, lambda need, rows: rng.randrange(0, need + 2)))


# ---- the select rule (sregex_amd/csrc/sre_lines_select.h): the entry table from the lines' records ----

DECLINED, ERROR = -5, -1        # SRE_DECLINED, SRE_ERROR (include/sregex/sregex.h)


def make_records(gspans, lens, G, rc=0):
    """records of 2 + 2 (G + 1) words as the scanner leaves them: rc, a word no rule reads, the match (group 0) and
    groups 1 .. G ((-1, -1): unset).  None: a line without a match, whose spans hold numbers that must not be read"""
    recs = []
    for sp, n in zip(gspans, lens):
        if sp is None:
            recs += [DECLINED, 77] + [0, 0] * (G + 1)
        else:
            recs += [rc, 77, 0, n] + [x for g in sp for x in (g if g is not None else (-1, -1))]
    return recs, 4 + 2 * G


def select_words(esim, recs, slots, st, lens, all_lines, groups):
    n, K = len(st), len(groups)
    val, start = (_u64 * (n * K))(), (_u64 * (n * K))()
    esim.lesim_select((_i64 * len(recs))(*recs), slots, n, DECLINED, int(all_lines), (_u64 * n)(*st), (_u64 * n)(*lens),
                      (_u32 * K)(*groups), K, val, start)
    return list(val), list(start)


@pytest.mark.parametrize("groups", [[2], [3, 1, 2]])
def test_the_select_rule_writes_the_entry_table(esim, groups):
    """K = 1 (FIRST and LAST on one entry) and K = 3: lines without a match, unset groups, empty groups at offset 0 and
    at len, empty lines"""
    rng = random.Random(46 + len(groups))
    G = 3
    lines = [b"", b"", b"abcdef", b"abcdef", b"xy", text(rng, 9)]
    gspans = [[(0, 0)] * 3, None, [(0, 0), (6, 6), (2, 5)], [None, (1, 3), None], None, [None, None, None]]
    for _ in range(6):
        ln = text(rng, rng.randrange(0, 30))
        sp = []
        for _ in range(G):
            a = rng.randrange(0, len(ln) + 1)
            sp.append(None if rng.random() < 0.25 else (a, rng.randrange(a, len(ln) + 1)))
        lines.append(ln)
        gspans.append(sp if rng.random() < 0.7 else None)
    lens = [len(ln) for ln in lines]
    st = [sum(lens[:i]) + i for i in range(len(lines))]
    recs, slots = make_records(gspans, lens, G)
    spans = [None if sp is None else [sp[g - 1] for g in groups] for sp in gspans]
    for all_lines in (False, True):
        val, starts, _ = entry_table(esim, lines, spans, len(groups), all_lines)
        assert select_words(esim, recs, slots, st, lens, all_lines, groups) == (val, starts), (groups, all_lines)


def test_the_select_rule_on_hostile_records(esim):
    """spans no scanner should leave, and an rc that is neither a regex id nor SRE_DECLINED: the literal words, and no
    start word outside its line"""
    LAST, UNSET, FIRST = esim.lesim_flag_last(), esim.lesim_flag_unset(), esim.lesim_flag_first()
    n, both = 10, FIRST | LAST
    # (rc, the span of group 1) -> (val, start - st) of the one entry
    unset = (1, UNSET | both)
    cases = [((0, (-3, 4)), unset), ((0, (5, 3)), unset), ((0, (2, n + 1)), unset), ((0, (2, 2 ** 62)), unset),
             ((0, (-2 ** 63, 2 ** 63 - 1)), unset), ((0, (-1, -1)), unset), ((0, (n, n)), (1, n | both)),
             ((0, (0, n)), (n + 1, both)), ((ERROR, (2, 5)), (4, 2 | both)), ((ERROR, (2, n + 1)), unset),
             ((7, (n + 1, n + 1)), unset), ((DECLINED, (2, 5)), (0, UNSET | both))]
    st = [100 + 40 * i for i in range(len(cases))]
    recs = [x for (rc, sp), _ in cases for x in (rc, 77, 0, n) + sp]
    for all_lines in (False, True):
        val, start = select_words(esim, recs, 6, st, [n] * len(cases), all_lines, [1])
        for i, ((rc, sp), (v, w)) in enumerate(cases):
            want = (1 if all_lines and rc == DECLINED else v, st[i] + w)
            assert (val[i], start[i]) == want, (rc, sp, all_lines, val[i], hex(start[i]))
            assert st[i] <= start[i] & (FIRST - 1) <= st[i] + n
    # two fields of one line: FIRST on the one, LAST on the other, each with its own verdict
    val, start = select_words(esim, [0, 77, 0, n, 4, n + 1, 4, n], 8, [100], [n], False, [1, 2])
    assert (val, start) == ([1, n - 4 + 1], [100 | UNSET | FIRST, 104 | LAST])
