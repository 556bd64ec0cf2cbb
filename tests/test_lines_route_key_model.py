"""The partition of the line route by key (sre_hip_route_lines_by_key) on the CPU: tests/lines_route_key_sim.cpp runs count,
scan and scatter of every digit pass workgroup by workgroup and slot by slot with the rules the kernels compile
(sregex_amd/csrc/sre_lines_route_key.h, sre_lines_route.h) and counts every store.  After pass p the items must be sorted
stably by their low p digits, after the last one by (key, line); every word of every array is written exactly once per
pass; the two rank rules of a slot give the same ranks; heads and bucket rows equal itertools.groupby; the cut and the totals
hold at every capacity; and fed through the extract's gather model (tests/lines_extract_sim.cpp, unchanged) every output
byte is written once.  A case is a list of lines and, per line, its key id (a dictionary row, -1 or -2)."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32, _i64, _u8 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint8
_p64, _p32, _p8, _pi64 = ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(_u8), ctypes.POINTER(_i64)
FILL = 0xA5
DELIM = 0x0A
BITS, TURNS = 0, 1          # SRE_LRK_RANK_BITS, SRE_LRK_RANK_TURNS


def _build(name, source, headers):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, source)] + [os.path.join(csrc, h) for h in headers]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def ksim():
    L = _build("liblinesroutekeysim.so", "lines_route_key_sim.cpp", ["sre_lines_route_key.h", "sre_lines_route.h", "sre_lines_gather.h"])
    for name in ("lrksim_flags", "lrksim_start_mask", "lrksim_max_lines", "lrksim_dropped"):
        getattr(L, name).restype = _u64
    L.lrksim_items.restype = _u32
    L.lrksim_sort_key.restype = _i64
    L.lrksim_sort_key.argtypes = [_i64, _u64, ctypes.c_int]
    L.lrksim_key_id.restype = _i64
    L.lrksim_key_id.argtypes = [_u64, _u64]
    L.lrksim_item.restype = _u64
    L.lrksim_item.argtypes = [_u64, _u64]
    L.lrksim_digit_bits.restype = _u32
    L.lrksim_digit_bits.argtypes = [ctypes.c_long]
    L.lrksim_max_key.restype = _u64
    L.lrksim_max_key.argtypes = [_u64, ctypes.c_int]
    L.lrksim_passes.restype = _u32
    L.lrksim_passes.argtypes = [_u64, _u32]
    L.lrksim_slot.restype = _u32
    L.lrksim_slot.argtypes = [_p8, _p32, _u32, ctypes.c_int, _p32, _p32]
    L.lrksim_count.restype = None
    L.lrksim_count.argtypes = [_pi64, _p64, _u64, _u64, ctypes.c_int, _u32, _u32, ctypes.c_int, _p64, _p32]
    L.lrksim_scan.restype = None
    L.lrksim_scan.argtypes = [_p64, _u64]
    L.lrksim_scatter.restype = _u64
    L.lrksim_scatter.argtypes = [_pi64, _p64, _u64, _u64, ctypes.c_int, _u32, _u32, ctypes.c_int, _p64, _u64, _p64, _p32]
    L.lrksim_table.restype = None
    L.lrksim_table.argtypes = [_p64, _p64, _u64, _u64, _p64, _p64, _p64, _p32]
    L.lrksim_heads.restype = None
    L.lrksim_heads.argtypes = [_p64, _p64, _u64, _p64, _p32]
    L.lrksim_bucket_row.restype = None
    L.lrksim_bucket_row.argtypes = [_p64, _p64, _u64, _p64, _u64, _pi64]
    L.lrksim_index_row.restype = None
    L.lrksim_index_row.argtypes = [_p64, _p64, _p64, _u64, _u64, _pi64]
    L.lrksim_cut.restype = _u64
    L.lrksim_cut.argtypes = [_p64, _u64, _u64]
    return L


@pytest.fixture(scope="module")
def gsim():
    """the extract's gather model, as tests/test_lines_extract_model.py builds it (a library of its own here)"""
    L = _build("liblinesextractsim_route_key.so", "lines_extract_sim.cpp", ["sre_lines_gather.h"])
    L.lesim_gather.restype = _u64
    L.lesim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32,
                               _p64, _p64]
    return L


def make_lines(rng, n, longest=8):
    return [bytes(rng.choice(b"abcxyz .") for _ in range(rng.randrange(longest + 1))) for _ in range(n)]


def host_passes(max_key, bits):
    """the host rule, spelled out: the bits of the largest key (at least one), `bits` a pass"""
    return (max(max_key.bit_length(), 1) + bits - 1) // bits


def sort_key(i, rows, all_lines):
    if i >= 0:
        return i
    return None if not all_lines else rows if i == -1 else rows + 1


def partition(ksim, ids, rows, all_lines, bits, rule=BITS):
    """every pass of the model; returns the sorted items after asserting every pass"""
    n = len(ids)
    want_keys = [sort_key(i, rows, all_lines) for i in ids]
    for i, k in zip(ids, want_keys):
        assert ksim.lrksim_sort_key(i, rows, all_lines) == (-1 if k is None else k)
    max_key = ksim.lrksim_max_key(rows, all_lines)
    assert max_key == (rows + 1 if all_lines else max(rows - 1, 0))
    assert all(k is None or k <= max_key for k in want_keys)
    passes = ksim.lrksim_passes(max_key, bits)
    assert passes == host_passes(max_key, bits), "the number of passes is the one the host rule gives"
    line_order = [(k << 32) | i for i, k in enumerate(want_keys) if k is not None]
    items_wg, nd = ksim.lrksim_items(), 1 << bits
    a_ids = (_i64 * max(n, 1))(*ids)
    src, nsrc = None, n
    for p in range(passes):
        nwg = (nsrc + items_wg - 1) // items_wg
        ncnt = nd * nwg
        cnt, cw = (_u64 * (ncnt + 1))(), (_u32 * (ncnt + 1))()
        if nsrc:
            ksim.lrksim_count(a_ids if p == 0 else None, src, nsrc, rows, all_lines, p, bits, rule, cnt, cw)
        assert list(cw)[:ncnt] == [1] * ncnt, "every count word exactly once"
        ksim.lrksim_scan(cnt, ncnt)
        total = cnt[ncnt]
        assert total == len(line_order), (p, total)
        dst, dw = (_u64 * (total + 1))(), (_u32 * (total + 1))()
        if nsrc and total:
            assert ksim.lrksim_scatter(a_ids if p == 0 else None, src, nsrc, rows, all_lines, p, bits, rule, cnt, total, dst, dw) == 0
        assert list(dw) == [1] * total + [0], "every item slot exactly once per pass"
        # stable by the low (p + 1) digits: Python's sort is stable, the items start in line order
        low = (1 << ((p + 1) * bits)) - 1
        assert list(dst)[:total] == sorted(line_order, key=lambda it: (it >> 32) & low), (p, bits)
        src, nsrc = dst, total
    got = list(src)[:nsrc]
    assert got == sorted(line_order), "sorted by (key, line)"
    return got, passes


def tail(ksim, gsim, lines, items, rows, src_off=0, dst_off=0, caps=(None,)):
    """the compact table, the heads, the bucket rows, the cut, the index rows and the gather over the sorted items"""
    n, nsel = len(lines), len(items)
    d = bytes([DELIM])
    buf = b"".join(ln + d for ln in lines)
    ends, pos = [], 0
    for ln in lines:
        ends.append(pos + len(ln))
        pos += len(ln) + 1
    a_items, a_ends = (_u64 * max(nsel, 1))(*items), (_u64 * max(n, 1))(*ends)
    cstart, coff, head = (_u64 * max(nsel, 1))(), (_u64 * (nsel + 1))(), (_u64 * (nsel + 1))()
    tw = (_u32 * max(nsel, 1))()
    ksim.lrksim_table(a_items, a_ends, nsel, n, cstart, coff, head, tw)
    assert list(tw)[:nsel] == [1] * nsel
    order = [it & 0xFFFFFFFF for it in items]
    flags, mask = ksim.lrksim_flags(), ksim.lrksim_start_mask()
    for r, i in enumerate(order):
        assert cstart[r] & ~mask == flags and cstart[r] & mask == ends[i] - len(lines[i]) and coff[r] == len(lines[i]) + 1
    groups = [(k, [it & 0xFFFFFFFF for it in g]) for k, g in itertools.groupby(items, key=lambda it: it >> 32)]
    heads = []
    for _, g in groups:
        heads += [1] + [0] * (len(g) - 1)
    assert list(head)[:nsel] == heads, "the heads equal itertools.groupby"
    ksim.lrksim_scan(head, nsel)
    ksim.lrksim_scan(coff, nsel)
    nbuckets = head[nsel]
    assert nbuckets == len(groups)
    texts = [lines[i] + d for i in order]
    need = sum(len(t) for t in texts)
    assert coff[nsel] == need
    hrank, hw = (_u64 * (nsel + 1))(), (_u32 * (nsel + 1))()
    ksim.lrksim_heads(a_items, head, nsel, hrank, hw)
    assert list(hw) == ([1] * (nbuckets + 1) + [0] * (nsel - nbuckets) if nsel else [0])
    rank = 0
    for b, (k, g) in enumerate(groups):
        row = (_i64 * 5)()
        ksim.lrksim_bucket_row(a_items, hrank, b, coff, rows, row)
        nbytes = sum(len(lines[i]) + 1 for i in g)
        assert list(row) == [k if k < rows else rows - 1 - k, rank, len(g), coff[rank], nbytes], (b, list(row))
        assert g == sorted(g)
        rank += len(g)
    for r in (0, nsel // 2, nsel - 1) if nsel else ():
        row = (_i64 * 5)()
        ksim.lrksim_index_row(a_items, cstart, coff, r, rows, row)
        k, i = items[r] >> 32, order[r]
        assert list(row) == [i, ends[i] - len(lines[i]), len(lines[i]), coff[r], k if k < rows else rows - 1 - k]
    src_len = (src_off + len(buf) + 15) // 16 * 16
    src = bytes([0xEE]) * src_off + buf + bytes([0xEE]) * (src_len - src_off - len(buf))
    for cap in caps:
        cap = need if cap is None else cap(need, [len(t) for t in texts])
        if cap < 0:
            continue
        want, k = b"", 0
        for t in texts:
            if len(want) + len(t) > cap:
                break
            want += t
            k += 1
        cut = ksim.lrksim_cut(coff, nsel, cap) if nsel else 0
        assert cut == k, (cap, cut, k)
        out_bytes = coff[cut] if nsel else 0
        assert out_bytes == len(want) <= cap
        if out_bytes == 0:
            continue        # (the call launches no gather)
        dst_len = (dst_off + out_bytes + 15) // 16 * 16
        dst = (_u8 * dst_len)(*([FILL] * dst_len))
        reads, writes = (_u32 * max(src_len, 1))(), (_u32 * dst_len)()
        win, glo = _u64(), _u64()
        bad = gsim.lesim_gather(coff, cstart, nsel, out_bytes, src_off, dst_off, DELIM, DELIM, src, src_len, dst, dst_len, reads,
                                writes, ctypes.byref(win), ctypes.byref(glo))
        ctx = (n, rows, src_off, dst_off, cap, out_bytes)
        assert bad == 0, ("accesses outside the aligned extents", bad, ctx)
        got = bytes(dst)
        assert got[dst_off:dst_off + out_bytes] == want, ctx
        w = list(writes)
        assert w[dst_off:dst_off + out_bytes] == [1] * out_bytes, ("every output byte exactly once", ctx)
        assert not any(w[:dst_off]) and not any(w[dst_off + out_bytes:]), ("a write outside [out, out + out_bytes)", ctx)
        assert got[:dst_off] == bytes([FILL]) * dst_off and got[dst_off + out_bytes:] == bytes([FILL]) * (dst_len - dst_off - out_bytes)


# need, need - 1, one row, 0
CAPS = (None, lambda need, rows: need - 1, lambda need, rows: rows[0] if rows else 0, lambda need, rows: 0)

SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
RANGES = (1, 2, 255, 256, 257, 70000)
WIDTHS = (1, 4, 8)


def one_key(rng, n, rows):
    return [rows - 1] * n, False


def round_robin(rng, n, rows):
    return [i % rows for i in range(n)], False


def every_key_distinct(rng, n, rows):
    """(as far as the range goes: beyond it the ids wrap)"""
    step = max(rows // max(n, 1), 1)
    return [(i * step) % rows for i in range(n)], False


def descending(rng, n, rows):
    return [(n - 1 - i) % rows for i in range(n)], False


def random_third_dropped(rng, n, rows):
    return [rng.choice((-1, -2)) if rng.random() < 1 / 3 else rng.randrange(rows) for _ in range(n)], False


def all_dropped(rng, n, rows):
    return [rng.choice((-1, -2)) for _ in range(n)], False


def rest_buckets(rng, n, rows):
    """ALL: the ids -1 and -2 become the keys rows and rows + 1"""
    return [rng.choice((-1, -2)) if rng.random() < 1 / 3 else rng.randrange(rows) for _ in range(n)], True


DISTRIBUTIONS = (one_key, round_robin, every_key_distinct, descending, random_third_dropped, all_dropped, rest_buckets)


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("rows", RANGES)
@pytest.mark.parametrize("dist", DISTRIBUTIONS, ids=lambda f: f.__name__)
def test_partition(ksim, gsim, dist, rows, bits):
    for n in SIZES:
        rng = random.Random(n * 1000 + rows * 7 + bits)
        ids, all_lines = dist(rng, n, rows)
        items, passes = partition(ksim, ids, rows, all_lines, bits)
        if n in (65, 1025, 5000) and (bits == 8 or rows <= 257):
            # the other rank rule gives the same items pass by pass (partition asserts every pass against Python)
            assert partition(ksim, ids, rows, all_lines, bits, rule=TURNS) == (items, passes)
        if bits == 8 or n in (65, 1025):
            tail(ksim, gsim, make_lines(rng, n), items, rows, src_off=rng.randrange(16), dst_off=rng.randrange(16))


def test_passes():
    assert [host_passes(k, 8) for k in (0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 30) + 1)] == [1, 1, 2, 2, 3, 3, 4, 4]


def test_the_host_rules(ksim):
    assert ksim.lrksim_max_lines() == (1 << 32) - 1
    assert [ksim.lrksim_digit_bits(v) for v in (-1, 0, 1, 2, 5, 8, 9, 64)] == [8, 8, 1, 2, 5, 8, 8, 8]
    # sets of 1, 200, 4096, 200 000 and 2^20 rows at the default width; 300 rows at 1, 2 and 5 bits
    assert [ksim.lrksim_passes(ksim.lrksim_max_key(r, 0), 8) for r in (0, 1, 200, 4096, 200000, 1 << 20, 1 << 30)] == [1, 1, 1, 2, 3, 3, 4]
    assert [ksim.lrksim_passes(ksim.lrksim_max_key(r, 1), 8) for r in (0, 254, 255, 256, 257, 65534, 65535)] == [1, 1, 2, 2, 2, 2, 3]
    assert [ksim.lrksim_passes(ksim.lrksim_max_key(300, a), b) for b in (1, 2, 5) for a in (0, 1)] == [9, 9, 5, 5, 2, 2]
    # ids and keys
    assert [ksim.lrksim_sort_key(i, 10, 0) for i in (0, 9, 10, -1, -2, -3)] == [0, 9, -1, -1, -1, -1]
    assert [ksim.lrksim_sort_key(i, 10, 1) for i in (0, 9, 10, -1, -2, -3)] == [0, 9, -1, 10, 11, -1]
    assert [ksim.lrksim_key_id(k, 10) for k in (0, 9, 10, 11)] == [0, 9, -1, -2]
    assert ksim.lrksim_item((1 << 30) + 1, (1 << 32) - 2) != ksim.lrksim_dropped()


@pytest.mark.parametrize("bits", (1, 2, 3, 4, 5, 6, 7, 8))
def test_both_rank_rules_give_the_same_ranks(ksim, bits):
    rng = random.Random(bits)
    nd = 1 << bits
    for trial in range(60):
        spread = rng.choice((1, 2, 3, nd))
        digit = [rng.randrange(min(spread, nd)) if spread < nd else rng.randrange(nd) for _ in range(64)]
        if trial % 7 == 0:
            digit = [(x * 5) % nd for x in range(64)]       # as many distinct digits as the width allows
        sel = [0 if rng.random() < (0.3 if trial % 3 else 0.0) else 1 for _ in range(64)]
        if trial == 59:
            sel = [0] * 64
        a_sel, a_digit = (_u8 * 64)(*sel), (_u32 * 64)(*digit)
        got = {}
        for rule in (BITS, TURNS):
            rank, c = (_u32 * 64)(), (_u32 * nd)()
            ballots = ksim.lrksim_slot(a_sel, a_digit, bits, rule, rank, c)
            distinct = len({d for d, s in zip(digit, sel) if s})
            assert ballots == (bits if rule == BITS else distinct), "the cost rule"
            got[rule] = (list(rank), list(c))
        want_rank = [sum(1 for y in range(x) if sel[y] and digit[y] == digit[x]) if sel[x] else 0 for x in range(64)]
        want_c = [sum(1 for y in range(64) if sel[y] and digit[y] == d) for d in range(nd)]
        assert got[BITS] == got[TURNS] == (want_rank, want_c)


@pytest.mark.parametrize("n", (1, 65, 1025, 2049))
@pytest.mark.parametrize("rows", (1, 5, 257))
def test_cuts(ksim, gsim, n, rows):
    rng = random.Random(n * 11 + rows)
    lines = make_lines(rng, n)
    ids = [rng.randrange(rows) for _ in range(n)]
    lines[0], ids[0] = b"first line", 0             # (the first row of the output, so "one row" is a real capacity)
    for all_lines in (False, True):
        items, _ = partition(ksim, ids, rows, all_lines, 8)
        tail(ksim, gsim, lines, items, rows, src_off=2, dst_off=13, caps=CAPS)


def test_empty_lines_and_a_long_one(ksim, gsim):
    rng = random.Random(5)
    lines = make_lines(rng, 300, longest=3)
    lines[17] = bytes(rng.choice(b"abc") for _ in range(20000))
    for i in range(0, 300, 9):
        lines[i] = b""
    ids = [i % 3 if i % 5 else -2 for i in range(300)]
    for all_lines in (False, True):
        items, _ = partition(ksim, ids, 3, all_lines, 8)
        tail(ksim, gsim, lines, items, 3, src_off=4, dst_off=11, caps=CAPS)
