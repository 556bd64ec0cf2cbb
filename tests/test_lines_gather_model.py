"""The gather of the line filter (sre_hip_filter_lines) on the CPU: tests/lines_gather_sim.cpp walks every output
chunk with the chunk logic the kernel compiles (sregex_amd/csrc/sre_lines_gather.h), tile by tile with the kernel's
table slices and LDS window rule, and counts every source byte read and every output byte written.  Expected
output is Python's b"".join(line + delim)."""
import bisect
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32 = ctypes.c_uint64, ctypes.c_uint32
_p64, _p32, _p8 = ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_uint8)
FILL = 0xA5


@pytest.fixture(scope="module")
def gsim():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "liblinesgathersim.so")
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, "lines_gather_sim.cpp"), os.path.join(csrc, "sre_lines_gather.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    L = ctypes.CDLL(so)
    L.lgsim_tile_chunks.restype = _u32
    L.lgsim_window.restype = _u32
    L.lgsim_gather.restype = _u64
    L.lgsim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32, _p64, _p64]
    L.lgsim_plan.restype = _u32
    L.lgsim_plan.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u64, _p64, _u32, _p64]
    return L


def table(lines, selected, final_delim=True):
    """(buffer, ends, off) of a line buffer as the runtime holds them after the split and the scan"""
    delim = b"\n"
    buf = delim.join(lines) + (delim if final_delim and lines else b"")
    ends, pos = [], 0
    for ln in lines:
        ends.append(pos + len(ln))
        pos += len(ln) + 1
    off = [0]
    for ln, s in zip(lines, selected):
        off.append(off[-1] + (len(ln) + 1 if s else 0))
    return buf, ends, off


def run(gsim, lines, selected, src_off, dst_off, final_delim=True, out_cap=None, delim=0x0A):
    """the model over one table; asserts where it reads and writes and what it writes; returns (windowed, global) tiles"""
    d = bytes([delim])
    lines = [ln.replace(d, b"?") for ln in lines]
    buf, ends, off = table(lines, selected, final_delim)
    buf = buf.replace(b"\n", d) if delim != 0x0A else buf
    n = len(lines)
    want = b""
    for ln, s in zip(lines, selected):
        if s:
            if out_cap is not None and len(want) + len(ln) + 1 > out_cap:
                break
            want += ln + d
    out_bytes = len(want)
    src_len = (src_off + len(buf) + 15) // 16 * 16
    src = bytes([0xEE]) * src_off + buf + bytes([0xEE]) * (src_len - src_off - len(buf))
    dst_len = (dst_off + out_bytes + 15) // 16 * 16
    dst = (ctypes.c_uint8 * max(dst_len, 1))(*([FILL] * max(dst_len, 1)))
    reads = (_u32 * max(src_len, 1))()
    writes = (_u32 * max(dst_len, 1))()
    win, glo = _u64(), _u64()
    bad = gsim.lgsim_gather((_u64 * (n + 1))(*off), (_u64 * max(n, 1))(*ends), n, out_bytes, src_off, dst_off, delim, src, src_len,
                            dst, dst_len, reads, writes, ctypes.byref(win), ctypes.byref(glo))
    ctx = (len(lines), src_off, dst_off, out_bytes)
    assert bad == 0, ("accesses outside the aligned extents", bad, ctx)
    got = bytes(dst)[:dst_len]
    assert got[dst_off:dst_off + out_bytes] == want, ctx
    w = list(writes)[:dst_len]
    assert w[dst_off:dst_off + out_bytes] == [1] * out_bytes, ("every output byte exactly once", ctx)
    assert not any(w[:dst_off]) and not any(w[dst_off + out_bytes:]), ("a write outside [out, out + out_bytes)", ctx)
    assert got[:dst_off] == bytes([FILL]) * dst_off and got[dst_off + out_bytes:] == bytes([FILL]) * (dst_len - dst_off - out_bytes)
    return win.value, glo.value


def text(rng, n):
    return bytes(rng.choice(b"abcdefgh@. ") for _ in range(n))


def test_hand_made_tables(gsim):
    rng = random.Random(7)
    lens = [0, 1, 15, 16, 17, 31, 32, 33]
    cases = [
        ([b""] * 40, [True] * 40),                                      # all lines empty
        ([b""] * 40, [i % 3 == 0 for i in range(40)]),
        ([text(rng, k) for k in lens], [True] * len(lens)),
        ([text(rng, k) for k in lens], [i % 2 == 0 for i in range(len(lens))]),
        ([text(rng, k) for k in lens], [i % 2 == 1 for i in range(len(lens))]),
        ([text(rng, k) for k in lens * 3], [True] * (3 * len(lens))),
        ([text(rng, 40000)], [True]),                                   # one long line over several tiles
        ([text(rng, 5), text(rng, 40000), b"", text(rng, 3)], [False, True, True, True]),
        ([text(rng, 20)] * 5, [False] * 5),                             # nothing selected
    ]
    for lines, sel in cases:
        for so, do in [(0, 0), (1, 0), (0, 1), (7, 9), (15, 15), (3, 8)]:
            for final in (True, False):
                run(gsim, lines, sel, so, do, final)


def test_window_and_global_table_paths(gsim):
    """a tile with more lines than the LDS window holds (empty selected lines: one line per output byte; and runs of
    unselected lines) searches the global table; the usual tile takes the window"""
    rng = random.Random(8)
    W = gsim.lgsim_window()
    win, glo = run(gsim, [b""] * (3 * W + 5), [True] * (3 * W + 5), 3, 5)
    assert glo >= 1, (win, glo)
    lines = [text(rng, 90) for _ in range(400)]
    win, glo = run(gsim, lines, [True] * 400, 2, 11)
    assert glo == 0 and win >= 2, (win, glo)
    # one selected line in front of and one behind a long run of unselected ones, inside one tile
    lines = [text(rng, 30)] + [b"x"] * (2 * W) + [text(rng, 30)]
    win, glo = run(gsim, lines, [True] + [False] * (2 * W) + [True], 5, 1)
    assert glo == 1 and win == 0, (win, glo)
    # exactly the window and one more
    for cnt in (W, W + 1):
        win, glo = run(gsim, [b""] * cnt, [True] * cnt, 0, 0)
        assert (win, glo) == ((1, 0) if cnt == W else (0, 1)), (cnt, win, glo)


def test_random_tables_every_alignment(gsim):
    rng = random.Random(int(os.environ.get("SRE_FUZZ_SEED", "20261017")) + 23)
    combos = [(s, d) for s in range(16) for d in range(16)]
    extra = [(rng.randrange(16), rng.randrange(16)) for _ in range(64)]
    for k, (so, do) in enumerate(combos + extra):
        big = k % 40 == 0
        nlines = rng.choice([1, 2, 3, 10, 60]) if not big else rng.choice([300, 1500])
        style = rng.randrange(4)
        lines = []
        for _ in range(nlines):
            if style == 0:
                n = rng.choice([0, 0, 1, 2, 15, 16, 17])
            elif style == 1:
                n = rng.randrange(0, 70)
            elif style == 2:
                n = rng.choice([0, 1, 33, 200, 700])
            else:
                n = rng.choice([0, 5, 16, 32, 48, 4100 if nlines < 20 else 100])
            lines.append(text(rng, n))
        p = rng.choice([0.0, 0.1, 0.5, 0.9, 1.0])
        sel = [rng.random() < p for _ in lines]
        need = sum(len(ln) + 1 for ln, s in zip(lines, sel) if s)
        cap = None if k % 3 else rng.randrange(0, need + 2)
        run(gsim, lines, sel, so, do, final_delim=bool(k & 1), out_cap=cap, delim=rng.choice([0x0A, 0x0A, 0, 255]))


def plan_reference(off, ends, out_bytes, src_head, dst_head, c):
    """the pieces of output chunk c byte by byte, in Python integers"""
    rows, first, count = [], None, 0
    for k in range(16):
        p = 16 * c + k
        o = p - dst_head
        if o < 0 or o >= out_bytes:
            continue
        first = k if first is None else first
        count += 1
        i = bisect.bisect_right(off, o) - 1
        start = ends[i - 1] + 1 if i else 0
        if o == off[i + 1] - 1:
            rows.append([1, 0, k, 1])
        else:
            s = src_head + start + (o - off[i])
            if rows and rows[-1][0] == 0 and rows[-1][1] + rows[-1][3] == s and rows[-1][4] == i:
                rows[-1][3] += 1
            else:
                rows.append([0, s, k, 1, i])
    return [r[:4] for r in rows], first, count


def test_offsets_beyond_32_bits_keep_64_bits(gsim):
    """a synthetic table only (no data): lines of several GiB, output offsets above 2^32, chunks planned one by one"""
    G = 1 << 30
    lens = [5 * G + 3, 0, 7, 6 * G + 11, 0, 0, 9 * G, 1, 40]
    sel = [True, True, False, True, True, False, True, True, True]
    ends, pos = [], 0
    for n in lens:
        ends.append(pos + n)
        pos += n + 1
    off = [0]
    for n, s in zip(lens, sel):
        off.append(off[-1] + (n + 1 if s else 0))
    out_bytes = off[-1]
    assert out_bytes > 1 << 34 and ends[-1] > 1 << 34
    T = gsim.lgsim_tile_chunks()
    a_off, a_ends = (_u64 * len(off))(*off), (_u64 * len(ends))(*ends)
    for src_head, dst_head in [(0, 0), (5, 11), (15, 1)]:
        nchunks = (dst_head + out_bytes + 15) // 16
        chunks = {0, 1, nchunks - 1, nchunks - 2, (1 << 28) + 1, (1 << 29) + 12345}
        for i in range(1, len(off)):
            for o in (off[i] - 17, off[i] - 1, off[i], off[i] + 16):
                if 0 <= o < out_bytes:
                    chunks.add((o + dst_head) // 16)
        for c in sorted(chunks):
            rows = (_u64 * (4 * 40))()
            fc = (_u64 * 4)()
            n = gsim.lgsim_plan(a_off, a_ends, len(lens), out_bytes, src_head, dst_head, c, rows, 40, fc)
            want, first, count = plan_reference(off, ends, out_bytes, src_head, dst_head, c)
            got = [list(rows[4 * j:4 * j + 4]) for j in range(n)]
            assert got == want, (src_head, dst_head, c, got, want)
            assert (fc[0], fc[1]) == (first, count)
            # the tile's slice holds the lines of its first and last byte
            t = c // T
            o_lo = max(t * T * 16, dst_head) - dst_head
            o_hi = min((t + 1) * T * 16, dst_head + out_bytes) - dst_head
            assert fc[2] == bisect.bisect_right(off, o_lo) - 1 and fc[3] == bisect.bisect_right(off, o_hi - 1) - 1
    assert any(r > 1 << 32 for r in off)
