"""The line sort (sre_hip_sort_lines) on the CPU: tests/lines_sort_sim.cpp runs the values pass and count, scan and scatter of
every digit pass workgroup by workgroup and slot by slot with the rules the kernels compile (sregex_amd/csrc/sre_lines_sort.h,
sre_lines_route_key.h, sre_lines_route.h, sre_lines_sums.h) and counts every store.  The key rule holds at its edges; the pass
count follows the range; after pass p the items must be sorted stably by their low p digits, after the last one by (key,
line); every word of every item array is written exactly once per pass; the cut and the totals hold at every limit and
capacity; and fed through the extract's gather model (tests/lines_extract_sim.cpp, unchanged) every output byte is written
once.  A case is a list of (text of the line, field) with field = (offset, length) of the sort group, "unset", or None for a
line without a match."""
import ctypes
import os
import random
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32, _i64, _u8, _i8, _i32 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint8, ctypes.c_int8, ctypes.c_int32
_p64, _p32, _p8, _pi64, _pi8 = (ctypes.POINTER(t) for t in (_u64, _u32, _u8, _i64, _i8))
_int = ctypes.c_int
FILL = 0xA5
DELIM = 0x0A
BIG = 10 ** 18 - 1
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
NUMBER = re.compile(rb"-?[0-9]{1,18}")


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
def ssim():
    L = _build("liblinessortsim.so", "lines_sort_sim.cpp",
               ["sre_lines_sort.h", "sre_lines_sums.h", "sre_lines_route_key.h", "sre_lines_route.h", "sre_lines_gather.h"])
    for name in ("lsosim_flags", "lsosim_start_mask", "lsosim_unset", "lsosim_dropped"):
        getattr(L, name).restype = _u64
    L.lsosim_items.restype = _u32
    L.lsosim_values_lines.restype = _u32
    L.lsosim_range.restype = _u64
    L.lsosim_range.argtypes = [_u64, _i64, _i64]
    L.lsosim_selected.restype = _u64
    L.lsosim_selected.argtypes = [_u64, _u64, _int]
    L.lsosim_max_key.restype = _u64
    L.lsosim_max_key.argtypes = [_u64, _u64, _u64, _int]
    L.lsosim_passes.restype = _u32
    L.lsosim_passes.argtypes = [_u64, _u64, _u64, _int]
    L.lsosim_limited.restype = _u64
    L.lsosim_limited.argtypes = [_u64, _u64]
    L.lsosim_digit.restype = _u32
    L.lsosim_digit.argtypes = [_u64, _u32]
    L.lsosim_key.restype = _u64
    L.lsosim_key.argtypes = [_i32, _i64, _i64, _i64, _u64, _int, _int]
    L.lsosim_values.restype = _u64
    L.lsosim_values.argtypes = [ctypes.c_char_p, _u64, _p64, _p64, _u64, _pi64, _pi8, _p32, _p32, _p64, _p32]
    L.lsosim_count.restype = None
    L.lsosim_count.argtypes = [_pi64, _pi8, _p64, _u64, _i64, _i64, _u64, _int, _int, _u32, _p64, _p32]
    L.lsosim_scan.restype = None
    L.lsosim_scan.argtypes = [_p64, _u64]
    L.lsosim_scatter.restype = _u64
    L.lsosim_scatter.argtypes = [_pi64, _pi8, _p64, _p32, _u64, _i64, _i64, _u64, _int, _int, _u32, _p64, _u64, _p64, _p32, _p32, _p32]
    L.lsosim_table.restype = None
    L.lsosim_table.argtypes = [_p32, _p64, _u64, _u64, _p64, _p64, _p32]
    L.lsosim_result.restype = None
    L.lsosim_result.argtypes = [_p64, _u64, _u64, _p64]
    L.lsosim_index_row.restype = None
    L.lsosim_index_row.argtypes = [_u64, _p64, _p64, _u64, _i64, _i32, _pi64]
    return L


@pytest.fixture(scope="module")
def gsim():
    """the extract's gather model, as tests/test_lines_extract_model.py builds it (a library of its own here)"""
    L = _build("liblinesextractsim_sort.so", "lines_extract_sim.cpp", ["sre_lines_gather.h"])
    L.lesim_gather.restype = _u64
    L.lesim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32,
                               _p64, _p64]
    return L


def host_passes(max_key):
    """the host rule, spelled out: the bits of the largest key (at least one), 8 a pass"""
    return (max(max_key.bit_length(), 1) + 7) // 8


def classify(text, field):
    """(class, value) of a line in pure Python"""
    if field is None:
        return -2, 0
    if field == "unset":
        return -1, 0
    a, ln = field
    t = text[a:a + ln]
    return (1, int(t)) if NUMBER.fullmatch(t) else (-1, 0)


def line_of(rng, v, pad=None):
    """a line `<pad> v=<v> <pad>` and its field"""
    pad = bytes(rng.choice(b"abcxyz .") for _ in range(rng.randrange(6))) if pad is None else pad
    t = str(v).encode() if not isinstance(v, bytes) else v
    return pad + b"v=" + t + b" " + pad, (len(pad) + 2, len(t))


def layout(case):
    d = bytes([DELIM])
    buf = b"".join(t + d for t, _ in case)
    ends, pos = [], 0
    for t, _ in case:
        ends.append(pos + len(t))
        pos += len(t) + 1
    return buf, ends


def values_pass(ssim, case):
    """the values pass of the model against classify; returns (values, classes, totals)"""
    n = len(case)
    buf, ends = layout(case)
    flags, unset = ssim.lsosim_flags(), ssim.lsosim_unset()
    vval, vstart = (_u64 * max(n, 1))(), (_u64 * max(n, 1))()
    for i, (t, f) in enumerate(case):
        st = ends[i] - len(t)
        if f is None:
            vval[i], vstart[i] = 0, st | unset | flags
        elif f == "unset":
            vval[i], vstart[i] = 1, st | unset | flags
        else:
            vval[i], vstart[i] = f[1] + 1, (st + f[0]) | flags
    value, cls = (_i64 * max(n, 1))(), (_i8 * max(n, 1))()
    vw, cw = (_u32 * max(n, 1))(), (_u32 * max(n, 1))()
    totals, sent = (_u64 * 4)(), (_u32 * 4)()
    assert ssim.lsosim_values(buf, len(buf), vval, vstart, n, value, cls, vw, cw, totals, sent) == 0
    want = [classify(t, f) for t, f in case]
    assert list(zip(cls, value))[:n] == want
    assert list(vw)[:n] == [1] * n and list(cw)[:n] == [1] * n, "value and class of every line exactly once"
    nums = [v for c, v in want if c == 1]
    keyed = sum(1 for c, _ in want if c != -2)
    vmin, vmax = ctypes.c_int64(totals[2]).value, ctypes.c_int64(totals[3]).value
    assert (totals[0], totals[1], vmin, vmax) == (keyed, len(nums), min(nums, default=I64_MAX), max(nums, default=I64_MIN))
    per = ssim.lsosim_values_lines()
    groups = [want[w:w + per] for w in range(0, n, per)]
    with_key = sum(1 for g in groups if any(c != -2 for c, _ in g))
    with_num = sum(1 for g in groups if any(c == 1 for c, _ in g))
    assert list(sent) == [with_key, with_num, with_num, with_num], "at most one add, minimum and maximum per workgroup"
    return value, cls, (keyed, len(nums), vmin, vmax)


def py_key(c, v, vmin, vmax, nnum, desc, all_lines):
    rng = vmax - vmin if nnum else 0
    if c == 1:
        return vmax - v if desc else v - vmin
    return rng + 1 if all_lines else None


def sort_passes(ssim, case, desc, all_lines):
    """the values pass and every digit pass of the model; returns (lines in output order, values, classes, totals, passes)"""
    n = len(case)
    value, cls, (keyed, nnum, vmin, vmax) = values_pass(ssim, case)
    rng = ssim.lsosim_range(nnum, vmin, vmax)
    assert rng == (vmax - vmin if nnum else 0) and rng < 1 << 61
    want_keys = [py_key(cls[i], value[i], vmin, vmax, nnum, desc, all_lines) for i in range(n)]
    dropped = ssim.lsosim_dropped()
    for i, k in enumerate(want_keys):
        assert ssim.lsosim_key(cls[i], value[i], vmin, vmax, nnum, desc, all_lines) == (dropped if k is None else k)
    items = [(k, i) for i, k in enumerate(want_keys) if k is not None]
    nsel = ssim.lsosim_selected(n, nnum, all_lines)
    assert nsel == len(items)
    max_key = ssim.lsosim_max_key(n, nnum, rng, all_lines)
    assert max_key == max((k for k, _ in items), default=max_key) or not items
    passes = ssim.lsosim_passes(n, nnum, rng, all_lines)
    assert passes == (host_passes(max_key) if items else 0)
    per = ssim.lsosim_items()
    src, sline, nsrc = None, None, n
    for p in range(passes):
        nwg = (nsrc + per - 1) // per
        ncnt = 256 * nwg
        cnt, cw = (_u64 * (ncnt + 1))(), (_u32 * (ncnt + 1))()
        first = p == 0
        ssim.lsosim_count(value if first else None, cls if first else None, src, nsrc, vmin, vmax, nnum, desc, all_lines, p, cnt, cw)
        assert list(cw)[:ncnt] == [1] * ncnt, "every count word exactly once"
        ssim.lsosim_scan(cnt, ncnt)
        total = cnt[ncnt]
        assert total == nsel, (p, total)
        dkey, dline = (_u64 * (total + 1))(), (_u32 * (total + 1))()
        kw, lw = (_u32 * (total + 1))(), (_u32 * (total + 1))()
        assert ssim.lsosim_scatter(value if first else None, cls if first else None, src, sline, nsrc, vmin, vmax, nnum, desc,
                                   all_lines, p, cnt, total, dkey, dline, kw, lw) == 0
        assert list(kw) == [1] * total + [0] and list(lw) == [1] * total + [0], "every word of both item arrays exactly once per pass"
        low = (1 << ((p + 1) * 8)) - 1
        # stable by the low (p + 1) digits: Python's sort is stable, the items start in line order
        assert list(zip(dkey, dline))[:total] == sorted(items, key=lambda it: it[0] & low), (p, n)
        src, sline, nsrc = dkey, dline, total
    got = list(zip(src, sline))[:nsel] if passes else []
    assert got == sorted(items), "sorted by (key, line)"
    # ... which is the order the header promises
    sign = -1 if desc else 1
    numbered = sorted((i for i in range(n) if cls[i] == 1), key=lambda i: (sign * value[i], i))
    rest = [i for i in range(n) if cls[i] != 1] if all_lines else []
    assert [i for _, i in got] == numbered + rest
    return [i for _, i in got], value, cls, (keyed, nnum, vmin, vmax), passes


def tail(ssim, gsim, case, order, value, cls, limits=(0,), caps=(None,), src_off=0, dst_off=0):
    """the compact table in front of the limit, the result words, the index rows and the gather over the sorted lines"""
    n, nsel = len(case), len(order)
    buf, ends = layout(case)
    a_lines, a_ends = (_u32 * max(nsel, 1))(*order), (_u64 * max(n, 1))(*ends)
    flags, mask = ssim.lsosim_flags(), ssim.lsosim_start_mask()
    src_len = (src_off + len(buf) + 15) // 16 * 16
    src = bytes([0xEE]) * src_off + buf + bytes([0xEE]) * (src_len - src_off - len(buf))
    for limit in limits:
        nout = ssim.lsosim_limited(nsel, limit)
        assert nout == (min(limit, nsel) if limit else nsel)
        cstart, coff, tw = (_u64 * max(nout, 1))(), (_u64 * (nout + 1))(), (_u32 * max(nout, 1))()
        ssim.lsosim_table(a_lines, a_ends, nout, n, cstart, coff, tw)
        assert list(tw)[:nout] == [1] * nout
        for r in range(nout):
            i = order[r]
            assert cstart[r] & ~mask == flags and cstart[r] & mask == ends[i] - len(case[i][0]) and coff[r] == len(case[i][0]) + 1
        ssim.lsosim_scan(coff, nout)
        texts = [case[i][0] + bytes([DELIM]) for i in order[:nout]]
        need = sum(len(t) for t in texts)
        for r in (0, nout // 2, nout - 1) if nout else ():
            row, i = (_i64 * 6)(), order[r]
            ssim.lsosim_index_row(i, cstart, coff, r, value[i], cls[i], row)
            assert list(row) == [i, ends[i] - len(case[i][0]), len(case[i][0]), coff[r], value[i] if cls[i] == 1 else 0, cls[i]]
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
            res = (_u64 * 4)()
            ssim.lsosim_result(coff, nout, cap, res)
            assert list(res) == [nout, need, k, len(want)], (limit, cap, list(res))
            out_bytes = res[3]
            if out_bytes == 0:
                continue        # (the call launches no gather)
            dst_len = (dst_off + out_bytes + 15) // 16 * 16
            dst = (_u8 * dst_len)(*([FILL] * dst_len))
            reads, writes = (_u32 * max(src_len, 1))(), (_u32 * dst_len)()
            win, glo = _u64(), _u64()
            bad = gsim.lesim_gather(coff, cstart, nout, out_bytes, src_off, dst_off, DELIM, DELIM, src, src_len, dst, dst_len, reads,
                                    writes, ctypes.byref(win), ctypes.byref(glo))
            ctx = (n, limit, src_off, dst_off, cap, out_bytes)
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


def status_codes(rng, n):
    return [line_of(rng, rng.choice((200, 200, 200, 301, 404, 500, 599))) for _ in range(n)]


def all_equal(rng, n):
    return [line_of(rng, -42) for _ in range(n)]


def sixteen_bits(rng, n):
    return [line_of(rng, rng.randrange(65536)) for _ in range(n)]


def below_2_24(rng, n):
    return [line_of(rng, rng.randrange(1 << 24)) for _ in range(n)]


def bits_32_to_39(rng, n):
    """values that differ ONLY in bits 32 .. 39: a 32-bit digit shift sorts nothing"""
    return [line_of(rng, (rng.randrange(256) << 32) + 12345) for _ in range(n)]


def top_digit(rng, n):
    """values that differ only in the top digit of an 8-pass range: a dropped last pass sorts nothing"""
    return [line_of(rng, rng.randrange(8) << 56) for _ in range(n)]


def full_range(rng, n):
    return [line_of(rng, rng.choice((BIG, -BIG, 0, rng.randrange(-BIG, BIG + 1)))) for _ in range(n)]


def descending_input(rng, n):
    return [line_of(rng, n - i) for i in range(n)]


def mixed_classes(rng, n):
    """a third of the lines is not numbered: no match, an unset group, or a text that is no number"""
    out = []
    for _ in range(n):
        x = rng.random()
        if x < 0.1:
            t, _f = line_of(rng, 7)
            out.append((t, None))
        elif x < 0.2:
            t, _f = line_of(rng, 7)
            out.append((t, "unset"))
        elif x < 0.33:
            out.append(line_of(rng, rng.choice((b"+1", b"1 ", b"-", b"", b"1234567890123456789", b"12a", b"--1"))))
        else:
            out.append(line_of(rng, rng.choice((b"-0", b"007", str(rng.randrange(-300, 300)).encode()))))
    return out


def none_numbered(rng, n):
    return [(line_of(rng, b"x")[0], rng.choice((None, "unset"))) if rng.random() < 0.5 else line_of(rng, b"abc") for _ in range(n)]


DISTRIBUTIONS = (status_codes, all_equal, sixteen_bits, below_2_24, bits_32_to_39, top_digit, full_range, descending_input,
                 mixed_classes, none_numbered)


@pytest.mark.parametrize("all_lines", (0, 1), ids=("numbered", "all"))
@pytest.mark.parametrize("desc", (0, 1), ids=("asc", "desc"))
@pytest.mark.parametrize("dist", DISTRIBUTIONS, ids=lambda f: f.__name__)
def test_sort(ssim, gsim, dist, desc, all_lines):
    for n in SIZES:
        rng = random.Random(n * 1000 + desc * 7 + all_lines)
        case = dist(rng, n)
        order, value, cls, _, _ = sort_passes(ssim, case, desc, all_lines)
        if n in (65, 1025, 5000):
            tail(ssim, gsim, case, order, value, cls, src_off=rng.randrange(16), dst_off=rng.randrange(16))


def test_the_passes_follow_the_data(ssim):
    rng = random.Random(1)
    got = {}
    for dist in (all_equal, status_codes, sixteen_bits, below_2_24, bits_32_to_39, top_digit, full_range):
        case = dist(rng, 300)
        if dist is below_2_24:
            case[0], case[1] = line_of(rng, 0), line_of(rng, (1 << 24) - 1)
        if dist is full_range:
            case[0], case[1] = line_of(rng, BIG), line_of(rng, -BIG)
        got[dist.__name__] = sort_passes(ssim, case, 0, 0)[4]
    assert got == {"all_equal": 1, "status_codes": 2, "sixteen_bits": 2, "below_2_24": 3, "bits_32_to_39": 5, "top_digit": 8,
                   "full_range": 8}


def test_the_pass_count(ssim):
    ranges = (0, 255, 256, (1 << 16) - 1, 1 << 24, 1 << 32, 1 << 56, 2 * BIG)
    assert [ssim.lsosim_passes(10, 10, r, 0) for r in ranges] == [1, 1, 2, 2, 4, 5, 8, 8]
    assert [host_passes(r) for r in ranges] == [1, 1, 2, 2, 4, 5, 8, 8]
    # ALL with a line that is not numbered: the rest key range + 1 may take a digit more; with none it does not
    assert [ssim.lsosim_passes(10, 9, r, 1) for r in ranges] == [1, 2, 2, 3, 4, 5, 8, 8]
    assert [ssim.lsosim_passes(10, 10, r, 1) for r in ranges] == [1, 1, 2, 2, 4, 5, 8, 8]
    # nothing selected: no pass; no numbered line under ALL: every key is the rest key 1, one pass
    assert ssim.lsosim_passes(10, 0, 0, 0) == 0 and ssim.lsosim_passes(0, 0, 0, 1) == 0
    assert ssim.lsosim_passes(10, 0, 0, 1) == 1
    # the digit shift reaches 56 on the 64-bit key
    key = 0x0123456789ABCDEF
    assert [ssim.lsosim_digit(key, p) for p in range(8)] == [0xEF, 0xCD, 0xAB, 0x89, 0x67, 0x45, 0x23, 0x01]


def test_the_key_rule_at_the_edges(ssim):
    dropped = ssim.lsosim_dropped()
    assert dropped == (1 << 64) - 1
    key = ssim.lsosim_key
    # vmin == vmax: every key 0, the rest key 1
    for v in (0, -5, BIG, -BIG):
        assert key(1, v, v, v, 3, 0, 0) == 0 and key(1, v, v, v, 3, 1, 0) == 0
        assert key(-1, 0, v, v, 3, 0, 1) == 1 and key(-2, 0, v, v, 3, 1, 1) == 1
    # the full range, both directions: computed in uint64_t, no signed overflow
    assert key(1, -BIG, -BIG, BIG, 2, 0, 0) == 0 and key(1, BIG, -BIG, BIG, 2, 0, 0) == 2 * BIG
    assert key(1, -BIG, -BIG, BIG, 2, 1, 0) == 2 * BIG and key(1, BIG, -BIG, BIG, 2, 1, 0) == 0
    assert key(1, 0, -BIG, BIG, 2, 0, 0) == BIG == key(1, 0, -BIG, BIG, 2, 1, 0)
    assert 2 * BIG + 1 < 1 << 61 and ssim.lsosim_range(2, -BIG, BIG) == 2 * BIG
    # the rest: behind every numbered line in both directions under ALL, dropped without
    for desc in (0, 1):
        assert key(-1, 0, -BIG, BIG, 2, desc, 1) == 2 * BIG + 1 == key(-2, 0, -BIG, BIG, 2, desc, 1)
        assert key(-1, 0, -BIG, BIG, 2, desc, 0) == dropped == key(-2, 0, -BIG, BIG, 2, desc, 0)
    # no numbered line: the identities are not subtracted
    assert ssim.lsosim_range(0, I64_MAX, I64_MIN) == 0
    assert key(-1, 0, I64_MAX, I64_MIN, 0, 0, 1) == 1 and key(-2, 0, I64_MAX, I64_MIN, 0, 1, 0) == dropped
    assert [ssim.lsosim_selected(10, 4, a) for a in (0, 1)] == [4, 10]
    assert [ssim.lsosim_limited(10, lim) for lim in (0, 1, 9, 10, 11, 1 << 40)] == [10, 1, 9, 10, 10, 10]


def test_the_number_rule_is_the_tallys(ssim):
    rng = random.Random(3)
    texts = (b"0", b"-0", b"007", b"-1", b"9" * 18, b"-" + b"9" * 18, b"9" * 19, b"-" + b"9" * 19, b"+1", b"1 ", b" 1", b"-", b"",
             b"1-", b"--1", b"1.5", b"1e3", b"0x10")
    case = [line_of(rng, t) for t in texts]
    _, cls, totals = values_pass(ssim, case)
    assert list(cls)[:len(texts)] == [1] * 6 + [-1] * 12
    assert totals == (18, 6, -BIG, BIG)


@pytest.mark.parametrize("n", (1, 65, 1025, 2049))
@pytest.mark.parametrize("dist", (status_codes, mixed_classes), ids=lambda f: f.__name__)
def test_limits_and_cuts(ssim, gsim, n, dist):
    rng = random.Random(n * 11)
    case = dist(rng, n)
    case[0] = (b"first line v=-400 ", (13, 4))         # (the first row ascending, so "one row" is a real capacity)
    for desc, all_lines in ((0, 0), (1, 0), (0, 1), (1, 1)):
        order, value, cls, totals, _ = sort_passes(ssim, case, desc, all_lines)
        nsel = len(order)
        # a limit in the middle of a run of equal values, when there is one
        mid = next((r for r in range(1, nsel) if cls[order[r]] == 1 and cls[order[r - 1]] == 1
                    and value[order[r]] == value[order[r - 1]]), max(nsel // 2, 1))
        tail(ssim, gsim, case, order, value, cls, limits=(0, 1, mid, nsel, nsel + 1, 1 << 40), caps=CAPS, src_off=2, dst_off=13)


def test_empty_lines_and_a_long_one(ssim, gsim):
    rng = random.Random(5)
    case = [line_of(rng, rng.randrange(-9, 9)) for _ in range(300)]
    case[17] = line_of(rng, 3, pad=bytes(rng.choice(b"abc") for _ in range(20000)))
    for i in range(0, 300, 9):
        case[i] = (b"", None)
    for all_lines in (0, 1):
        order, value, cls, _, _ = sort_passes(ssim, case, 1, all_lines)
        tail(ssim, gsim, case, order, value, cls, limits=(0, 40), caps=CAPS, src_off=4, dst_off=11)
