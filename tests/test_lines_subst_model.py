"""The gather of the line substitute (sre_hip_substitute_lines) on the CPU: tests/lines_subst_sim.cpp walks every
output chunk with the chunk logic the kernel compiles (sregex_amd/csrc/sre_lines_gather.h) over the piece table, tile
by tile with the kernel's table slices and LDS window rule, and counts every source byte and every byte of the literal
block read and every output byte written.  A case is a list of lines, per line None (no match) or a list of spans
(a, b) relative to the line, span 0 the match and span g group g (None: unset), and a template as a list of pieces:
bytes (a literal) or an int (a group).  Expected output is Python slicing."""
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
def ssim():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "liblinessubstsim.so")
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, "lines_subst_sim.cpp"), os.path.join(csrc, "sre_lines_gather.h"),
            os.path.join(csrc, "sre_lines_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    L = ctypes.CDLL(so)
    L.lssim_window.restype = _u32
    for f in (L.lssim_flag_last, L.lssim_flag_unset, L.lssim_flag_first, L.lssim_flag_literal):
        f.restype = _u64
    L.lssim_cut.restype = _u64
    L.lssim_cut.argtypes = [_p64, _u64, _u64, _u64]
    L.lssim_count.restype = _u64
    L.lssim_count.argtypes = [_p64, _u64, _u64]
    L.lssim_gather.restype = _u64
    L.lssim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, ctypes.c_char_p, _u64, ctypes.c_char_p, _u64, _p8, _u64,
                               _p32, _p32, _p32, _p64, _p64]
    L.lssim_select.restype = ctypes.c_int
    L.lssim_select.argtypes = [_pi64, _u32, _u64, _i64, ctypes.c_int, _p64, _p64, ctypes.POINTER(ctypes.c_int32), _p32, _p32, _u32,
                               _p64, _p64]
    return L


def piece_table(ssim, lines, spans, template, all_lines):
    """(val, starts, rows, literal block): the per-entry values and start words as the select pass leaves them, the
    expected row of every selected line and the literal bytes back to back, padded to a multiple of 16 with zeros"""
    LAST, UNSET, FIRST, LIT = ssim.lssim_flag_last(), ssim.lssim_flag_unset(), ssim.lssim_flag_first(), ssim.lssim_flag_literal()
    block, lit_off = b"", []
    for pc in template:
        lit_off.append(len(block))
        if isinstance(pc, bytes):
            assert pc
            block += pc
    block += bytes(-len(block) % 16)
    val, starts, rows, pos = [], [], [], 0
    for ln, sp in zip(lines, spans):
        selected = sp is not None or all_lines
        v, w = [], []
        if sp is None:
            v = [len(ln)] + [0] * len(template) + [1]
            w = [pos | FIRST | UNSET]
            for pc, lo in zip(template, lit_off):
                w.append(lo | LIT if isinstance(pc, bytes) else pos | UNSET)
            w.append((pos + len(ln)) | LAST)
            row = ln
        else:
            m0, m1 = sp[0]
            assert 0 <= m0 <= m1 <= len(ln)
            v, w, row = [m0], [pos | FIRST], ln[:m0]
            for pc, lo in zip(template, lit_off):
                if isinstance(pc, bytes):
                    v.append(len(pc))
                    w.append(lo | LIT)
                    row += pc
                elif sp[pc] is None:
                    v.append(0)
                    w.append(pos | UNSET)
                else:
                    a, b = sp[pc]
                    assert 0 <= a <= b <= len(ln)
                    v.append(b - a)
                    w.append(pos + a)
                    row += ln[a:b]
            v.append(len(ln) - m1 + 1)
            w.append((pos + m1) | LAST)
            row += ln[m1:]
        val += v if selected else [0] * len(v)
        starts += w
        if selected:
            rows.append(row)
        pos += len(ln) + 1
    return val, starts, rows, block


def run(ssim, lines, spans, template, src_off, dst_off, all_lines=False, caps=(None,), delim=0x0A):
    """the model over one table for every out_cap of `caps` (None: everything fits; a callable gets (need, row
    sizes)); asserts the cut, the counts of lines, where it reads and writes and what it writes; returns (windowed,
    global) of the last"""
    d = bytes([delim])
    assert not any(d in ln for ln in lines) and not any(d in pc for pc in template if isinstance(pc, bytes))
    buf = d.join(lines) + d
    n, P = len(lines), len(template) + 2
    val, starts, rows, block = piece_table(ssim, lines, spans, template, all_lines)
    off = [0]
    for v in val:
        off.append(off[-1] + v)
    nent = n * P
    need = off[-1]
    texts = [r + d for r in rows]
    assert sum(len(t) for t in texts) == need
    a_off, a_starts = (_u64 * (nent + 1))(*off), (_u64 * max(nent, 1))(*starts)
    assert ssim.lssim_count(a_off, P, n) == len(rows)                 # nselected, however many entries are empty
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
        i = ssim.lssim_cut(a_off, n, P, cap)
        out_bytes = off[i * P]
        assert out_bytes == len(want) <= cap, (cap, i, out_bytes, len(want))
        assert ssim.lssim_count(a_off, P, i) == k, (cap, i, k)       # nwritten
        dst_len = (dst_off + out_bytes + 15) // 16 * 16
        dst = (ctypes.c_uint8 * max(dst_len, 1))(*([FILL] * max(dst_len, 1)))
        reads = (_u32 * max(src_len, 1))()
        lit_reads = (_u32 * max(len(block), 1))()
        writes = (_u32 * max(dst_len, 1))()
        win, glo = _u64(), _u64()
        bad = ssim.lssim_gather(a_off, a_starts, nent, out_bytes, src_off, dst_off, delim, src, src_len, block, len(block), dst,
                                dst_len, reads, lit_reads, writes, ctypes.byref(win), ctypes.byref(glo))
        ctx = (n, P, src_off, dst_off, cap, out_bytes)
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


def matched_line(rng, glens, before=None, after=None):
    """a line whose match holds one group per length of `glens` in order (None: unset), filler between; `before` and
    `after`: the bytes in front of and behind the match.  Returns (line, spans)"""
    before = rng.randrange(0, 20) if before is None else before
    after = rng.randrange(0, 20) if after is None else after
    line = text(rng, before)
    groups = []
    for n in glens:
        if n is None:
            groups.append(None)
            continue
        line += text(rng, rng.randrange(0, 3))
        groups.append((len(line), len(line) + n))
        line += text(rng, n)
    m1 = len(line)
    return line + text(rng, after), [(before, m1)] + groups


TEMPLATES = {
    2: [],
    3: [1],
    5: [b"<", 1, b">"],
    32: [1, b"-", 2, 2, b"ab", 3, 1, b"0123456789abcdefXYZ", 2, 3, 3, 1] + [1, 2, 3] * 6,
}


@pytest.mark.parametrize("P", [2, 3, 5, 32])
def test_piece_counts_lengths_and_cuts(ssim, P):
    template = TEMPLATES[P]
    assert len(template) + 2 == P
    rng = random.Random(60 + P)
    lens = list(range(34))
    rng.shuffle(lens)
    lines, spans = [], []
    for r in range(0, 33, 3):
        ln, sp = matched_line(rng, lens[r:r + 3])
        lines.append(ln)
        spans.append(sp)
        if r % 2:
            lines.append(text(rng, rng.randrange(0, 40)))       # a line without a match: copied whole under ALL
            spans.append(None)
    for so, do in [(0, 0), (1, 0), (0, 1), (7, 9), (15, 15), (3, 8)]:
        for all_lines in (False, True):
            run(ssim, lines, spans, template, so, do, all_lines, CAPS)


def test_empty_prefix_suffix_match_and_whole_line(ssim):
    rng = random.Random(61)
    lines = [b"abcdef", b"abcdef", b"abcdef", b"abcdef", b"", b"abcdef", b"x"]
    spans = [[(0, 3), (1, 2)],          # no prefix
             [(2, 6), (2, 6)],          # no suffix
             [(3, 3), (3, 3)],          # an empty match: the replacement is inserted
             [(0, 6), None],            # the whole line, its group unset
             [(0, 0), (0, 0)],          # the empty line matches
             None,
             [(0, 1), (0, 1)]]
    for template in ([], [1], [b"<", 1, b">"], [1, 1, 0], [b"0123456789abcdefg"], [0]):
        for so, do in [(0, 0), (5, 11), (rng.randrange(16), rng.randrange(16))]:
            for all_lines in (False, True):
                run(ssim, lines, spans, template, so, do, all_lines, CAPS)


def test_empty_and_unset_pieces_between_pieces_that_take_bytes(ssim):
    rng = random.Random(62)
    lines, spans = [], []
    for k in range(40):
        g1 = [None, 0, 0, 5][k % 4]
        g2 = [None, 0, 7, None, 1][k % 5]
        ln, sp = matched_line(rng, [g1, g2])
        lines.append(ln)
        spans.append(sp)
    for template in ([1, 1, 2], [b"[", 1, 1, 2, b"]"], [1, b"|", 2, 2, 1, b"|", 1], [2, 1, 1, 1, 1, 2]):
        run(ssim, lines, spans, template, 3, 6, False, CAPS)
        run(ssim, lines, spans, template, 9, 2, True, CAPS)


def test_runs_of_empty_entries_take_the_window_or_the_global_table(ssim):
    rng = random.Random(63)
    W = ssim.lssim_window()
    # rows of 2 bytes with 3 empty entries of 5: a tile of 16 KiB meets far more than W entries
    nl = 3000
    lines = [b"k=1"] * nl
    spans = [[(0, 3), (2, 3), None, None]] * nl
    win, glo = run(ssim, lines, spans, [2, 1, 3], 3, 5, False, (None, lambda need, rows: need - 1, lambda need, rows: need // 2))
    assert win == 0 and glo >= 1
    # ... every third line without a match, under ALL (rows of 4 bytes between rows of 2) and without
    spans3 = [None if i % 3 == 1 else spans[i] for i in range(nl)]
    for all_lines in (True, False):
        win, glo = run(ssim, lines, spans3, [2, 1, 3], 1, 2, all_lines, (None, lambda need, rows: need - 1, 2 * 1024 + 1))
        assert win == 0 and glo >= 1
    # P = 32, all pieces empty: 32 entries for a row of 3 bytes
    spans32 = [[(0, 3), (3, 3), None, (1, 1)]] * 200
    win, glo = run(ssim, [b"k=1"] * 200, spans32, [1, 2, 3] * 10, 0, 0, False, tuple(reversed(CAPS)))
    assert (win, glo) == (0, 1)
    # fewer than W entries: the window
    win, glo = run(ssim, [b"xy"] * 100, [[(1, 1), None, (1, 1)]] * 100, [1, 2, 1], 1, 2)
    assert (win, glo) == (1, 0)
    # exactly the window and one entry more (P = 2: two entries a line)
    for cnt in (W // 2, W // 2 + 1):
        win, glo = run(ssim, [b""] * cnt, [[(0, 0)]] * cnt, [], 0, 0)
        assert (win, glo) == ((1, 0) if cnt == W // 2 else (0, 1)), (cnt, win, glo)
    # a run of unselected lines (no entry of theirs takes a byte) between two rows, inside one tile
    lines = [text(rng, 30)] + [b"x"] * W + [text(rng, 30)]
    spans = [[(3, 9), (4, 5)]] + [None] * W + [[(0, 30), (2, 2)]]
    win, glo = run(ssim, lines, spans, [b"<", 1, b">"], 5, 1)
    assert (win, glo) == (0, 1)
    win, glo = run(ssim, lines, spans, [b"<", 1, b">"], 5, 1, all_lines=True)
    assert (win, glo) == (0, 1)


@pytest.mark.parametrize("L", [1, 15, 16, 17, 33, 4096])
def test_literal_lengths_at_every_residue_of_the_block(ssim, L):
    """a literal of r bytes and a group in front put the literal under test at offset r of the literal block (the
    4096 bytes are all the block holds: with r in front the literal under test has 4096 - r)"""
    rng = random.Random(64 + L)
    lines, spans = [], []
    for n in (0, 3, 20):
        ln, sp = matched_line(rng, [n])
        lines.append(ln)
        spans.append(sp)
    lines.insert(1, b"no match")
    spans.insert(1, None)
    for r in range(16):
        lit = bytes(0x30 + (x * 7 + r) % 75 for x in range(L if L + r <= 4096 else L - r))
        template = ([b"x" * r] if r else []) + [1, lit]
        run(ssim, lines, spans, template, rng.randrange(16), rng.randrange(16), bool(r & 1), (None, lambda need, rows: need // 2))
        run(ssim, lines, spans, template + [0, lit[:1]], r, 15 - r)


def test_a_piece_of_40_kib_and_its_neighbours(ssim):
    rng = random.Random(65)
    big, sp = matched_line(rng, [3, 40 * 1024, 0], before=40 * 1024 + 5, after=33 * 1024)
    lines = [text(rng, 9), big, b"", text(rng, 40)]
    spans = [[(1, 4), (1, 2), None, (4, 4)], sp, None, [(0, 40), (0, 40), (40, 40), (39, 40)]]
    for so, do in [(0, 0), (5, 11), (15, 1)]:
        for template in ([2], [b"<", 2, 2, b">", 1, 3], []):
            run(ssim, lines, spans, template, so, do, False, CAPS)
            run(ssim, lines, spans, template, so, do, True, CAPS)


def test_every_alignment_pair(ssim):
    rng = random.Random(66)
    lines, spans = [], []
    for n in (0, 1, 5, 16, 17, 33, 2, 47):
        ln, sp = matched_line(rng, [n, rng.randrange(0, 4)])
        lines.append(ln)
        spans.append(sp if n != 2 else None)
    spans[3] = spans[3][:2] + [None]
    template = [b"0123456789abcdefg", 1, b"-", 2, 1]
    for so in range(16):
        for do in range(16):
            run(ssim, lines, spans, template, so, do, bool((so + do) & 1), (None, lambda need, rows: need // 2))


def test_unmatched_lines_between_matched_ones_and_other_delimiters(ssim):
    rng = random.Random(67)
    lines, spans = [], []
    for k in range(60):
        ln, sp = matched_line(rng, [rng.randrange(0, 20), None if k % 4 == 0 else rng.randrange(0, 5)])
        lines.append(ln.replace(b"\n", b"?").replace(b"\x00", b"?").replace(b"\xff", b"?"))
        spans.append(sp if rng.random() < 0.6 else None)
    for delim in (0x0A, 0, 255):
        for all_lines in (False, True):
            run(ssim, lines, spans, [b"[", 1, b"|", 2, b"]"], 4, 13, all_lines, CAPS, delim=delim)


def test_random_tables(ssim):
    rng = random.Random(int(os.environ.get("SRE_FUZZ_SEED", "20261018")) + 31)
    for k in range(60):
        np_ = rng.choice([0, 1, 2, 3, 6, 30])
        template = []
        for _ in range(np_):
            if rng.random() < 0.4 and not (template and isinstance(template[-1], bytes)):
                template.append(text(rng, rng.choice([1, 2, 15, 16, 17, 40])).replace(b"\n", b"?"))
            else:
                template.append(rng.randrange(0, 4))
        nlines = rng.choice([1, 2, 3, 10, 60]) if k % 15 else rng.choice([300, 1200])
        p = rng.choice([0.0, 0.1, 0.5, 0.9, 1.0])
        lines, spans = [], []
        for _ in range(nlines):
            ln = text(rng, rng.choice([0, 1, 15, 16, 17, 40, 90, 300])).replace(b"\n", b"?")
            m0 = rng.randrange(0, len(ln) + 1)
            sp = [(m0, rng.randrange(m0, len(ln) + 1))]
            for _ in range(3):
                if rng.random() < 0.3:
                    sp.append(None)
                else:
                    a = rng.randrange(0, len(ln) + 1)
                    sp.append((a, rng.randrange(a, len(ln) + 1)))
            lines.append(ln)
            spans.append(sp if rng.random() < p else None)
        run(ssim, lines, spans, template, rng.randrange(16), rng.randrange(16), bool(k & 1),
            (None, lambda need, rows: rng.randrange(0, need + 2)))


# ---- the select rule (sregex_amd/csrc/sre_lines_select.h): the piece table from the lines' records ----

DECLINED, ERROR = -5, -1        # SRE_DECLINED, SRE_ERROR (include/sregex/sregex.h)


def select_words(ssim, recs, slots, st, lens, all_lines, template):
    """the compiled rule over records of `slots` words (rc, a word no rule reads, then the spans of groups 0, 1, ..)"""
    pg, poff, plen, at = [], [], [], 0
    for pc in template:
        pg.append(-1 if isinstance(pc, bytes) else pc)
        poff.append(at if isinstance(pc, bytes) else 0)
        plen.append(len(pc) if isinstance(pc, bytes) else 0)
        at += len(pc) if isinstance(pc, bytes) else 0
    n, np_, P = len(st), len(template), len(template) + 2
    val, start = (_u64 * (n * P))(), (_u64 * (n * P))()
    assert ssim.lssim_select((_i64 * len(recs))(*recs), slots, n, DECLINED, int(all_lines), (_u64 * n)(*st), (_u64 * n)(*lens),
                             (ctypes.c_int32 * max(np_, 1))(*pg), (_u32 * max(np_, 1))(*poff), (_u32 * max(np_, 1))(*plen), np_,
                             val, start) == 0
    return list(val), list(start)


@pytest.mark.parametrize("template", [[], [b"<", 1, b"=", 2, b">"]])
def test_the_select_rule_writes_the_piece_table(ssim, template):
    """an empty template (P = 2) and one with literals, a set group and an unset group: lines without a match, empty
    groups at offset 0 and at len, empty lines"""
    rng = random.Random(70 + len(template))
    lines = [b"", b"", b"abcdef", b"abcdef", b"xy", b"abcdef"]
    spans = [[(0, 0), (0, 0), (0, 0)], None, [(0, 6), (0, 0), (6, 6)], [(2, 4), (2, 3), None], None, [(6, 6), None, None]]
    for _ in range(6):
        ln, sp = matched_line(rng, [rng.choice([None, 0, 1, 5]), rng.choice([None, 0, 2])])
        lines.append(ln)
        spans.append(sp if rng.random() < 0.7 else None)
    lens = [len(ln) for ln in lines]
    st = [sum(lens[:i]) + i for i in range(len(lines))]
    recs = []
    for sp in spans:
        recs += [DECLINED, 77] + [0, 0] * 3 if sp is None else [0, 77] + [x for g in sp for x in (g if g is not None else (-1, -1))]
    for all_lines in (False, True):
        val, starts, _, _ = piece_table(ssim, lines, spans, template, all_lines)
        assert select_words(ssim, recs, 8, st, lens, all_lines, template) == (val, starts), (template, all_lines)


def test_the_select_rule_on_hostile_records(ssim):
    """spans no scanner should leave, in match 0 (the line is copied whole, its pieces are empty) and in a group (the
    piece is unset), and an rc that is neither a regex id nor SRE_DECLINED: the literal words, and no start word outside
    its line or the literal block"""
    LAST, UNSET, FIRST, LIT = ssim.lssim_flag_last(), ssim.lssim_flag_unset(), ssim.lssim_flag_first(), ssim.lssim_flag_literal()
    n, template = 10, [b"ab", 1]
    # (rc, match 0, group 1) -> the four (val, start - st) of the line; a literal's start is its offset in the block
    whole = [(n, FIRST | UNSET), (0, LIT), (0, UNSET), (1, n | LAST)]
    piece_unset = [(2, FIRST), (2, LIT), (0, UNSET), (n - 6 + 1, 6 | LAST)]
    bad = [(-3, 4), (5, 3), (2, n + 1), (2, 2 ** 62), (-2 ** 63, 2 ** 63 - 1), (-1, -1)]
    cases = [((0, m, (2, 3)), whole) for m in bad] + [((0, (2, 6), g), piece_unset) for g in bad]
    cases += [((ERROR, (2, 6), (3, 5)), [(2, FIRST), (2, LIT), (2, 3), (5, 6 | LAST)]), ((ERROR, (2, n + 1), (3, 5)), whole),
              ((0, (n, n), (n, n)), [(n, FIRST), (2, LIT), (0, n), (1, n | LAST)]),
              ((0, (0, 0), (0, 0)), [(0, FIRST), (2, LIT), (0, 0), (n + 1, LAST)]), ((DECLINED, (2, 6), (3, 5)), whole)]
    st = [100 + 40 * i for i in range(len(cases))]
    recs = [x for (rc, m, g), _ in cases for x in (rc, 77) + m + g]
    for all_lines in (False, True):
        val, start = select_words(ssim, recs, 6, st, [n] * len(cases), all_lines, template)
        for i, ((rc, m, g), words) in enumerate(cases):
            for f, (v, w) in enumerate(words):
                want = (0 if rc == DECLINED and not all_lines else v, w if w & LIT else st[i] + w)
                assert (val[4 * i + f], start[4 * i + f]) == want, (rc, m, g, f, all_lines, val[4 * i + f], hex(start[4 * i + f]))
                assert w & LIT or st[i] <= start[4 * i + f] & (LIT - 1) <= st[i] + n
