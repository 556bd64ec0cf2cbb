"""The fold pass of the line fold (sre_hip_fold_lines) on the CPU: tests/lines_fold_sim.cpp runs marks, carry, apply, totals,
finish, record ids and records workgroup by workgroup with the block logic the kernels compile
(sregex_amd/csrc/sre_lines_fold.h) and the kernels' 1024 / 256 / 64 geometry.  Expected: a short loop in Python written from
the header's definitions, checked itself against a brute-force statement of them on 60 lines.  The entry table the model
leaves goes through the extract's gather model (tests/lines_extract_sim.cpp, the fields table), and the bytes must equal
Python's join."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32, _i64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
_p64, _p32, _pi64, _p8 = ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_uint8)
SIZE_MAX = (1 << 64) - 1
HEAD, LAST = 1, 2
FILL = 0xA5
N_BIG = 3 * 1024 + 17
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, N_BIG]


def build(name, source, headers):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, source)] + [os.path.join(csrc, h) for h in headers]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def fsim():
    L = build("liblinesfoldsim.so", "lines_fold_sim.cpp", ["sre_lines_fold.h", "sre_lines_context.h", "sre_lines_gather.h"])
    L.lfsim_items.restype = _u32
    L.lfsim_flag_last.restype = _u64
    L.lfsim_run.restype = _u64
    L.lfsim_run.argtypes = [_p64, _p64, _p64, _p64, _u64, ctypes.c_int, _u64, _p64, _p64, _p64, _pi64, _u64, _u64, _pi64, _p64]
    L.lfsim_carry.restype = None
    L.lfsim_carry.argtypes = [_p64, _p64, _u64]
    L.lfsim_marks_block.restype = _u64
    L.lfsim_marks_block.argtypes = [_p64, _u64, _u64, ctypes.c_int, _p64, _p64]
    L.lfsim_apply_block.restype = None
    L.lfsim_apply_block.argtypes = [_p64, _u64, _u64, ctypes.c_int, _u64, _u64, _u64, _p32, _p64, _p64]
    assert L.lfsim_items() == 1024 and L.lfsim_flag_last() == 1 << 63
    return L


@pytest.fixture(scope="module")
def esim():
    L = build("liblinesextractsim.so", "lines_extract_sim.cpp", ["sre_lines_gather.h", "sre_lines_select.h"])
    L.lesim_gather.restype = _u64
    L.lesim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32, _p64,
                               _p64]
    return L


def fold(marked, nxt, max_lines):
    """head(i) of every line, from the definitions: nh, the nearest natural head at or in front, the cap"""
    n, heads, h = len(marked), [], 0
    for i in range(n):
        nh = i == 0 or not (marked[i - 1] if nxt else marked[i])
        h = i if nh else h
        heads.append(nh or (max_lines != 0 and (i - h) % max_lines == 0))
    return heads


def by_definition(marked, nxt, max_lines):
    n = len(marked)
    nh = [i == 0 or not marked[i - (1 if nxt else 0)] for i in range(n)]
    out = []
    for i in range(n):
        h = max(j for j in range(i + 1) if nh[j])
        out.append(nh[i] or (max_lines != 0 and (i - h) % max_lines == 0))
    return out


def test_the_python_loop_is_the_definition():
    rng = random.Random(3)
    sets = [[False] * 60, [True] * 60, [k in (0, 7, 8, 30, 59) for k in range(60)], [k not in (0, 7, 8, 30, 59) for k in range(60)]]
    sets += [[rng.random() < p for _ in range(60)] for p in (0.1, 0.5, 0.9)]
    for m in sets:
        for nxt in (False, True):
            for cap in (0, 1, 2, 3, 7, 59, 60, 61, SIZE_MAX):
                assert fold(m, nxt, cap) == by_definition(m, nxt, cap)


def records_of(heads):
    """[(first line, lines)]"""
    firsts = [i for i, h in enumerate(heads) if h]
    return [(a, b - a) for a, b in zip(firsts, firsts[1:] + [len(heads)])]


def line_lengths(n, seed):
    rng = random.Random(seed)
    lens = [rng.randrange(0, 41) for _ in range(n)]
    ends, pos = [], 0
    for k in lens:
        ends.append(pos + k)
        pos += k + 1
    return lens, ends


def run(fsim, marked, lens, ends, nxt, max_lines, order=None, out_cap=SIZE_MAX, records_cap=None):
    """the model over one set of marked lines; asserts everything it writes; returns (off, start words, info)"""
    n = len(marked)
    nblk, nw = (n + 1023) // 1024, (n + 63) // 64
    heads = fold(marked, nxt, max_lines)
    recs = records_of(heads)
    val = (_u64 * (n + 1))(*([k + 1 if m else 0 for k, m in zip(lens, marked)] + [SIZE_MAX]))
    start, aux = (_u64 * n)(*([SIZE_MAX] * n)), (_u64 * n)(*([SIZE_MAX] * n))
    mbits, hbits = (_u64 * nw)(*([SIZE_MAX] * nw)), (_u64 * nw)(*([SIZE_MAX] * nw))
    recid = (_i64 * n)(*([-7] * n))
    rcap = len(recs) + 2 if records_cap is None else records_cap
    rows = (_i64 * (5 * rcap + 1))(*([-7] * (5 * rcap + 1)))
    info = (_u64 * 6)()
    order = list(range(nblk)) if order is None else order
    bad = fsim.lfsim_run(val, start, aux, (_u64 * n)(*ends), n, int(nxt), max_lines, (_u64 * nblk)(*order), mbits, hbits, recid,
                         out_cap, rcap, rows, info)
    ctx = (n, nxt, max_lines, [i for i, m in enumerate(marked) if m][:8])
    assert bad == 0, ("an access outside the workgroup's own lines", bad, ctx)
    # the bitmaps
    for bits, flags in ((mbits, marked), (hbits, heads)):
        want = [0] * nw
        for i in range(n):
            if flags[i]:
                want[i // 64] |= 1 << (i % 64)
        assert list(bits) == want, ctx
    # the entry table: every line, the delimiter behind the last line of a record
    off = [0]
    for k in lens:
        off.append(off[-1] + k + 1)
    assert list(val) == off, ctx
    starts = [e - k for e, k in zip(ends, lens)]
    last = [i == n - 1 or heads[i + 1] for i in range(n)]
    assert list(start) == [s | (1 << 63 if f else 0) for s, f in zip(starts, last)], ctx
    # aux: a head's next head, any other line's first line of its record
    want_aux, rid = [0] * n, [0] * n
    for r, (a, k) in enumerate(recs):
        want_aux[a] = a + k
        for i in range(a + 1, a + k):
            want_aux[i] = a
        for i in range(a, a + k):
            rid[i] = r
    assert list(aux) == want_aux, ctx
    assert list(recid) == rid, ctx
    # the cut: whole records only
    nwritten, out_bytes = 0, 0
    for a, k in recs:
        if off[a + k] > out_cap:
            break
        nwritten, out_bytes = nwritten + 1, off[a + k]
    assert tuple(info)[:5] == (len(recs), sum(marked), max(k for _, k in recs), nwritten, out_bytes), (tuple(info), ctx, out_cap)
    assert info[5] == (n if nwritten == len(recs) else recs[nwritten][0])
    nrows = min(rcap, nwritten)
    got = [tuple(rows[5 * r:5 * r + 5]) for r in range(nrows)]
    assert got == [(a, k, starts[a], off[a + k] - off[a] - 1, off[a]) for a, k in recs[:nrows]], ctx
    assert list(rows[5 * nrows:]) == [-7] * (5 * (rcap - nrows) + 1), ctx
    return off, list(start), info


def plants(n):
    """marked or unmarked lines at the edges of the buffer, of the waves and of the workgroups, alone and in pairs"""
    spots = [s for s in (0, 1, n - 2, n - 1, 254, 255, 256, 257, 1022, 1023, 1024, 1025, 2047, 2048) if 0 <= s < n]
    return [[s] for s in spots] + [[a, b] for a in spots for b in spots if a < b and b - a in (1, 2, 768, 769)] + [spots]


MODES = [(nxt, inv) for nxt in (False, True) for inv in (False, True)]


@pytest.mark.parametrize("n", SIZES)
def test_edges_of_buffer_wave_and_block(fsim, n):
    lens, ends = line_lengths(n, n)
    for spots in plants(n):
        base = [i in spots for i in range(n)]
        for nxt, inv in MODES:
            marked = [b != inv for b in base]
            for cap in (0, 3):
                run(fsim, marked, lens, ends, nxt, cap)


@pytest.mark.parametrize("n", SIZES)
def test_none_and_all_marked_and_random(fsim, n):
    lens, ends = line_lengths(n, n + 1)
    rng = random.Random(n)
    sets = [[False] * n, [True] * n] + [[rng.random() < p for _ in range(n)] for p in (0.03, 0.5, 0.97)]
    for marked in sets:
        for nxt in (False, True):
            for cap in (0, 5):
                run(fsim, marked, lens, ends, nxt, cap)


def test_one_record_over_more_than_two_blocks_in_any_block_order(fsim):
    n = N_BIG
    lens, ends = line_lengths(n, 9)
    rng = random.Random(9)
    for nxt in (False, True):
        # a record from line 700 to line 2900 (default: its continuation lines are marked; next: all but its last)
        marked = [rng.random() < 0.4 for _ in range(n)]
        for i in range(701 - nxt, 2901 - nxt):
            marked[i] = True
        marked[700 - nxt], marked[2901 - nxt] = False, False
        heads = fold(marked, nxt, 0)
        assert (700, 2201) in records_of(heads)
        for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
            _, _, info = run(fsim, marked, lens, ends, nxt, 0, order=order)
            assert info[2] == 2201
            run(fsim, marked, lens, ends, nxt, 1000, order=order)


@pytest.mark.parametrize("nxt,inv", MODES)
def test_max_lines(fsim, nxt, inv):
    n = N_BIG
    lens, ends = line_lengths(n, 5)
    rng = random.Random(5)
    sparse = [rng.random() < 0.002 for _ in range(n)]        # long records
    for base in (sparse, [False] * n, [i in (0, 1023, 1024, 2500) for i in range(n)]):
        marked = [b == inv for b in base]       # (inv False: nearly every line marked)
        for cap in (1, 2, 255, 256, 257, 1024, 1025, n, n + 1, 1 << 63, SIZE_MAX):
            run(fsim, marked, lens, ends, nxt, cap)


def test_the_carry_over_more_block_words_than_lanes(fsim):
    rng = random.Random(12)
    for nblk in (1, 2, 1023, 1024, 1025, 5000):
        last = [0] * nblk
        first = [SIZE_MAX] * nblk
        for b in range(nblk):
            if rng.random() < 0.3 or nblk < 3:
                a, z = sorted((rng.randrange(1025), rng.randrange(1025)))
                first[b], last[b] = (b << 10) + a, (b << 10) + z + 1
        l, f = (_u64 * nblk)(*last), (_u64 * nblk)(*first)
        fsim.lfsim_carry(l, f, nblk)
        hin, run_ = [], 0
        for b in range(nblk):
            hin.append(run_)
            run_ = max(run_, last[b])
        qin, run_ = [0] * nblk, SIZE_MAX
        for b in reversed(range(nblk)):
            qin[b] = run_
            run_ = min(run_, first[b])
        assert list(l) == hin and list(f) == qin, nblk


def test_a_block_beyond_two_to_the_32(fsim):
    rng = random.Random(21)
    base = (1 << 32) + 5 * 1024
    n = base + 1000                                     # the block is the last one, 1000 lines of it in the buffer
    for nxt in (False, True):
        for max_lines in (0, 3, 1 << 33):
            for hin, qin in [(0, SIZE_MAX), (base - 40 + 1, SIZE_MAX), ((1 << 32) - 9 + 1, SIZE_MAX), (base + (1 if nxt else 0), SIZE_MAX)]:
                marked = [rng.random() < 0.8 for _ in range(1000)]
                if hin == base + 1:
                    assert nxt          # (the head the last line of the block in front generated)
                v = (_u64 * 1024)(*([5 if m else 0 for m in marked] + [9] * 24))
                words, out = (_u64 * 17)(), (_u64 * 2)()
                assert fsim.lfsim_marks_block(v, base, n, int(nxt), words, out) == 0
                gen = [base + i + nxt for i, m in enumerate(marked) if not m]
                assert (out[0], out[1]) == ((gen[-1] + 1, gen[0]) if gen else (0, SIZE_MAX))
                fl, ax, counts = (_u32 * 1024)(), (_u64 * 1024)(), (_u64 * 3)()
                fsim.lfsim_apply_block(words, base, n, int(nxt), max_lines, hin, qin, fl, ax, counts)
                # the same lines with everything in front of them: hin (a P word) says where the nearest natural head is
                h0 = max(hin, 1) - 1
                heads, first, h = [], [], h0
                for i in range(1000):
                    g = base + i
                    nh = not (marked[i - 1] if nxt else marked[i]) if (i or not nxt) else hin == base + 1
                    h = g if nh else h
                    r = (g - h) % max_lines if max_lines else g - h
                    heads.append(r == 0)
                    first.append(g - r)
                assert [f & HEAD for f in fl][:1000] == [int(x) for x in heads], (nxt, max_lines, hin)
                assert [f for f in fl][1000:] == [0] * 24
                nexts = [base + i for i in range(1000) if heads[i]] + [n]
                for i in range(1000):
                    if heads[i]:
                        assert ax[i] == min(x for x in nexts if x > base + i)
                    else:
                        assert ax[i] == first[i]
                    assert bool(fl[i] & LAST) == (i == 999 or heads[i + 1])
                assert counts[0] == sum(heads) and counts[1] == sum(marked)


def test_out_cap_around_record_boundaries(fsim):
    n = 1500
    lens, ends = line_lengths(n, 17)
    rng = random.Random(17)
    marked = [rng.random() < 0.7 for _ in range(n)]
    for i in range(1000, 1100):
        marked[i] = True
    for nxt in (False, True):
        recs = records_of(fold(marked, nxt, 0))
        off = [0]
        for k in lens:
            off.append(off[-1] + k + 1)
        bounds = [off[a + k] for a, k in (recs[0], recs[len(recs) // 2], next(r for r in recs if r[1] >= 100))]
        for b in bounds:
            for cap in range(max(0, b - 45), b + 3):
                run(fsim, marked, lens, ends, nxt, 0, out_cap=cap, records_cap=3)
        for cap in (0, 1, off[-1] - 1, off[-1], off[-1] + 1):
            run(fsim, marked, lens, ends, nxt, 0, out_cap=cap)
        for rcap in (0, 1, len(recs) - 1, len(recs)):
            run(fsim, marked, lens, ends, nxt, 0, records_cap=rcap)


@pytest.mark.parametrize("n", [1, 5, 300, 1024, N_BIG])
def test_the_entry_table_gathers_to_the_python_join(fsim, esim, n):
    rng = random.Random(n)
    delim, join = 0x0A, 0x01
    lines = [bytes(rng.choice(b"xyw .") for _ in range(rng.randrange(0, 41))) for _ in range(n)]
    lens = [len(x) for x in lines]
    ends, pos = [], 0
    for k in lens:
        ends.append(pos + k)
        pos += k + 1
    buf = b"\n".join(lines) + b"\n"
    for nxt in (False, True):
        for max_lines in (0, 4):
            marked = [rng.random() < 0.6 for _ in range(n)]
            heads = fold(marked, nxt, max_lines)
            off, starts, info = run(fsim, marked, lens, ends, nxt, max_lines)
            want = b"".join(x + (b"\n" if i == n - 1 or heads[i + 1] else b"\x01") for i, x in enumerate(lines))
            assert want.count(b"\n") == info[0]
            for src_off, dst_off in [(0, 0), (3, 13)]:
                src_len = (src_off + len(buf) + 15) // 16 * 16
                src = bytes([0xEE]) * src_off + buf + bytes([0xEE]) * (src_len - src_off - len(buf))
                dst_len = (dst_off + len(want) + 15) // 16 * 16
                dst = (ctypes.c_uint8 * dst_len)(*([FILL] * dst_len))
                reads, writes = (_u32 * src_len)(), (_u32 * dst_len)()
                win, glo = _u64(), _u64()
                bad = esim.lesim_gather((_u64 * (n + 1))(*off), (_u64 * n)(*starts), n, len(want), src_off, dst_off, delim, join, src,
                                        src_len, dst, dst_len, reads, writes, ctypes.byref(win), ctypes.byref(glo))
                assert bad == 0
                got = bytes(dst)
                assert got[dst_off:dst_off + len(want)] == want
                assert got[:dst_off] == bytes([FILL]) * dst_off and got[dst_off + len(want):] == bytes([FILL]) * (dst_len - dst_off - len(want))
