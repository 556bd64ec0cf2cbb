"""The ordered tally (sre_hip_tally_top_lines) on the CPU: tests/lines_tally_top_sim.cpp runs the first lines, the order
values with their totals, the ordered table, the permute and the ranks lane by lane with the rules the kernels compile
(sregex_amd/csrc/sre_lines_tally_top.h); the digit passes between them are the line sort's model (lines_sort_sim.cpp through
lines_partition_sim.h) over the keys with all = 1.  The order value and the class hold for every `by`; the totals take at most
one atomic per word and workgroup; the range is refused exactly beyond 2^64 - 3; after the last pass the items are sorted by
(sort key, key number); every word of every caller array is written exactly once and nothing beyond the caps; fed through the
extract's gather model (tests/lines_extract_sim.cpp, unchanged) every output byte is written once; and the ranks of the lines
are the inverse of the item order.  Expected values are plain Python: sorted with key (+-value, k).

A case is (lines, aggs): lines[i] = (key number or None, text of the line, its K fields as (offset, length) or "unset"),
the key numbers in first-appearance order; aggs[k][c] = (sum, min, max, n) of key k and value column c."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32, _i64, _u8, _i8, _i32 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint8, ctypes.c_int8, ctypes.c_int32
_p64, _p32, _p8, _pi64, _pi8 = (ctypes.POINTER(t) for t in (_u64, _u32, _u8, _i64, _i8))
_int = ctypes.c_int
FILL = 0xA5
DELIM, FSEP = 0x0A, 0x09
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
COUNT, SUM, MIN, MAX, N = 0, 1, 2, 3, 4
BYS = ((COUNT, 0), (SUM, 0), (MIN, 0), (MAX, 1), (N, 1), (SUM, 1))
K, V = 2, 2
EMPTY = (1 << 64) - 1


def _build(name, source, headers):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, source)] + [os.path.join(csrc, h) for h in headers] + [os.path.join(HERE, "lines_sort_sim.cpp"),
                                                                                       os.path.join(HERE, "lines_partition_sim.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def tsim():
    L = _build("liblinestallytopsim.so", "lines_tally_top_sim.cpp",
               ["sre_lines_tally_top.h", "sre_lines_tally.h", "sre_lines_sort.h", "sre_lines_sums.h", "sre_lines_route_key.h",
                "sre_lines_route.h", "sre_lines_gather.h"])
    for name in ("lttsim_max_range", "lttsim_first_flag", "lttsim_last_flag", "lsosim_unset", "lsosim_start_mask", "lsosim_dropped"):
        getattr(L, name).restype = _u64
    for name in ("lttsim_keys", "lttsim_none", "lsosim_items"):
        getattr(L, name).restype = _u32
    L.lttsim_index_words.restype, L.lttsim_index_words.argtypes = _u32, [_u32]
    L.lttsim_by_ok.restype, L.lttsim_by_ok.argtypes = _int, [_int, _u64, _u64]
    L.lttsim_range_ok.restype, L.lttsim_range_ok.argtypes = _int, [_u64, _i64, _i64]
    L.lttsim_rows.restype, L.lttsim_rows.argtypes = _u64, [_u64, _u64]
    L.lttsim_passes.restype, L.lttsim_passes.argtypes = _u32, [_u64, _u64, _i64, _i64]
    L.lttsim_order.restype, L.lttsim_order.argtypes = _i32, [_int, _u64, _pi64, _pi64]
    L.lttsim_first.restype, L.lttsim_first.argtypes = _u64, [_p64, _p32, _p64, _u64, _u64, _p64, _p32]
    L.lttsim_values.restype, L.lttsim_values.argtypes = None, [_p64, _pi64, _u64, _u32, _int, _u32, _pi64, _pi8, _p32, _p64, _p32]
    L.lttsim_table.restype = _u64
    L.lttsim_table.argtypes = [_p32, _p64, _p64, _p64, _u64, _u64, _u64, _u32, _p64, _p64, _p32]
    L.lttsim_permute.restype = _u64
    L.lttsim_permute.argtypes = [_p32, _u64, _p64, _pi64, _u32, _p64, _p64, _u64, _p64, _p64, _u32, _pi64, _pi8, _p64, _u64, _p32,
                                 _pi64, _u64, _p32, _pi64, _u64, _p32, _p32, _p32]
    L.lttsim_ranks.restype, L.lttsim_ranks.argtypes = None, [_p32, _p64, _p32, _u64, _u64, _pi64, _p32]
    L.lsosim_key.restype = _u64
    L.lsosim_key.argtypes = [_i32, _i64, _i64, _i64, _u64, _int, _int]
    L.lsosim_count.restype = None
    L.lsosim_count.argtypes = [_pi64, _pi8, _p64, _u64, _i64, _i64, _u64, _int, _int, _u32, _p64, _p32]
    L.lsosim_scan.restype, L.lsosim_scan.argtypes = None, [_p64, _u64]
    L.lsosim_scatter.restype = _u64
    L.lsosim_scatter.argtypes = [_pi64, _pi8, _p64, _p32, _u64, _i64, _i64, _u64, _int, _int, _u32, _p64, _u64, _p64, _p32, _p32, _p32]
    return L


@pytest.fixture(scope="module")
def gsim():
    """the extract's gather model, as tests/test_lines_extract_model.py builds it (a library of its own here)"""
    L = _build("liblinesextractsim_top.so", "lines_extract_sim.cpp", ["sre_lines_gather.h"])
    L.lesim_gather.restype = _u64
    L.lesim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32,
                               _p64, _p64]
    return L


def make_case(rng, nkeys, spread=300, big=False, col1="some"):
    """nkeys keys, every one on 1 .. 3 lines (some on more: equal and different counts), lines without a key between them;
    column 0 holds a number on every keyed line, column 1 on the lines of some keys, of all or of none"""
    owners = []
    for k in range(nkeys):
        owners += [k] * (1 + (k * 7 + k // 3) % 3)
    head = list(range(nkeys))                   # first appearance in key order, the rest shuffled behind their first line
    rest = owners[:]
    for k in head:
        rest.remove(k)
    rng.shuffle(rest)
    order, pending = [], rest
    for k in head:
        order.append(k)
        while pending and pending[-1] <= k and rng.random() < 0.6:
            order.append(pending.pop())
        if rng.random() < 0.2:
            order.append(None)
    order += [k for k in pending]
    lines, aggs = [], [[[0, I64_MAX, I64_MIN, 0] for _ in range(V)] for _ in range(nkeys)]
    has1 = [col1 == "all" or (col1 == "some" and k % 3 != 1) for k in range(nkeys)]
    for k in order:
        if k is None:
            lines.append((None, b"no key here", None))
            continue
        key = b"key%d" % k
        a = rng.randrange(-10 ** 18 + 1, 10 ** 18) if big else rng.randrange(-spread, spread) // (1 + k % 4)
        b = rng.randrange(spread) if has1[k] else None
        text = key + b" a=%d b=%s" % (a, b"-" if b is None else b"%d" % b)
        f0 = (0, len(key))
        f1 = "unset" if k % 5 == 4 else (len(key) + 3, len(b"%d" % a))
        lines.append((k, text, (f0, f1)))
        for c, x in ((0, a), (1, b)):
            if x is not None:
                g = aggs[k][c]
                g[0] = (g[0] + x + (1 << 63)) % (1 << 64) - (1 << 63)
                g[1], g[2], g[3] = min(g[1], x), max(g[2], x), g[3] + 1
    return lines, aggs


def state(tsim, rng, case):
    """what the tally leaves on the device: the table, the slots of the lines, the key numbers in the counts' place, the counts,
    the aggregates, and the scanned entry table that selects the first line of every key"""
    lines, aggs = case
    n, nkeys = len(lines), len(aggs)
    none, flag_first, flag_last, unset = tsim.lttsim_none(), tsim.lttsim_first_flag(), tsim.lttsim_last_flag(), tsim.lsosim_unset()
    nslots = 1
    while nslots < 2 * max(nkeys, 1) + 7:
        nslots *= 2
    slots = rng.sample(range(nslots), nkeys)
    first, counts = [None] * nkeys, [0] * nkeys
    d = bytes([DELIM])
    buf, ends, pos = b"".join(t + d for _, t, _ in lines), [], 0
    val, start = [0] * (n * K), [0] * (n * K)
    for i, (k, t, fields) in enumerate(lines):
        ends.append(pos + len(t))
        if k is not None:
            counts[k] += 1
            kept = first[k] is None
            if kept:
                first[k] = i
            for f in range(K):
                flags = (flag_first if f == 0 else 0) | (flag_last if f == K - 1 else 0)
                if fields[f] == "unset":
                    start[i * K + f], ln = pos | unset | flags, 0
                else:
                    start[i * K + f], ln = (pos + fields[f][0]) | flags, fields[f][1]
                val[i * K + f] = ln + 1 if kept else 0
        pos += len(t) + 1
    off, run = [], 0
    for x in val:
        off.append(run)
        run += x
    off.append(run)
    tab, cnt = [EMPTY] * nslots, [0] * nslots
    for k in range(nkeys):
        tab[slots[k]], cnt[slots[k]] = first[k], k
    lslot = [none if k is None else slots[k] for k, _, _ in lines]
    flat = [w for k in range(nkeys) for c in range(V) for w in aggs[k][c]]
    return dict(n=n, nkeys=nkeys, buf=buf, ends=ends, first=first, counts=counts, off=off, start=start,
                a_tab=(_u64 * nslots)(*tab), a_cnt=(_u64 * nslots)(*cnt), a_lslot=(_u32 * max(n, 1))(*lslot),
                a_counts=(_u64 * max(nkeys, 1))(*counts), a_aggs=(_i64 * max(len(flat), 1))(*flat),
                a_off=(_u64 * (n * K + 1))(*off), a_start=(_u64 * max(n * K, 1))(*start), a_ends=(_u64 * max(n, 1))(*ends))


def py_order_value(by, col, count, agg):
    """(ordered, value) of a key in plain Python"""
    s, lo, hi, cnt = agg[col]
    if by == COUNT:
        return True, count
    if by == N:
        return True, cnt
    if cnt == 0:
        return False, 0
    return True, {SUM: s, MIN: lo, MAX: hi}[by]


def py_order(vals, desc):
    """the header's order: ordered keys by (+-value, k), then the others by k"""
    sign = -1 if desc else 1
    return sorted((k for k, (o, _) in enumerate(vals) if o), key=lambda k: (sign * vals[k][1], k)) + [k for k, (o, _) in enumerate(vals) if not o]


def run(tsim, gsim, rng, case, by, col, desc, limits=(0,), caps=((None, None, None, None),), cuts=(None,), src_off=0, dst_off=0,
        want_passes=None):
    st = state(tsim, rng, case)
    lines, aggs = case
    n, nkeys = st["n"], st["nkeys"]
    # 1. first lines
    first, fw = (_u64 * max(nkeys, 1))(), (_u32 * max(nkeys, 1))()
    assert tsim.lttsim_first(st["a_tab"], st["a_lslot"], st["a_cnt"], n, nkeys, first, fw) == 0
    assert list(first)[:nkeys] == st["first"] and list(fw)[:nkeys] == [1] * nkeys
    # 2. order values, classes, totals and the atomics sent
    value, cls, vw = (_i64 * max(nkeys, 1))(), (_i8 * max(nkeys, 1))(), (_u32 * max(nkeys, 1))()
    totals, sent = (_u64 * 4)(), (_u32 * 4)()
    tsim.lttsim_values(st["a_counts"], st["a_aggs"], nkeys, V, by, col, value, cls, vw, totals, sent)
    vals = [py_order_value(by, col, st["counts"][k], aggs[k]) for k in range(nkeys)]
    assert [(cls[k] == 1, value[k]) for k in range(nkeys)] == vals and set(list(cls)[:nkeys]) <= {1, -1}
    assert list(vw)[:nkeys] == [1] * nkeys
    ordered = [x for o, x in vals if o]
    vmin, vmax = ctypes.c_int64(totals[2]).value, ctypes.c_int64(totals[3]).value
    assert (totals[0], totals[1], vmin, vmax) == (nkeys, len(ordered), min(ordered, default=I64_MAX), max(ordered, default=I64_MIN))
    per = tsim.lttsim_keys()
    groups = [vals[w:w + per] for w in range(0, nkeys, per)]
    with_o = sum(1 for g in groups if any(o for o, _ in g))
    assert list(sent) == [len(groups), with_o, with_o, with_o], "at most one add, minimum and maximum per workgroup"
    nord = len(ordered)
    assert tsim.lttsim_range_ok(nord, vmin, vmax) == 1
    # 3. the digit passes over the keys, all = 1
    rng_ = vmax - vmin if nord else 0
    keys_want = [(vmax - x if desc else x - vmin) if o else rng_ + 1 for o, x in vals]
    for k in range(nkeys):
        assert tsim.lsosim_key(cls[k], value[k], vmin, vmax, nord, desc, 1) == keys_want[k] != tsim.lsosim_dropped()
    items = [(keys_want[k], k) for k in range(nkeys)]
    passes = tsim.lttsim_passes(nkeys, nord, vmin, vmax)
    assert passes == ((max(max(keys_want).bit_length(), 1) + 7) // 8 if nkeys else 0)
    if want_passes is not None:
        assert passes == want_passes
    items_per = tsim.lsosim_items()
    src, sline = None, None
    for p in range(passes):
        ncnt = 256 * ((nkeys + items_per - 1) // items_per)
        cnt, cw = (_u64 * (ncnt + 1))(), (_u32 * (ncnt + 1))()
        f = p == 0
        tsim.lsosim_count(value if f else None, cls if f else None, src, nkeys, vmin, vmax, nord, desc, 1, p, cnt, cw)
        assert list(cw)[:ncnt] == [1] * ncnt
        tsim.lsosim_scan(cnt, ncnt)
        assert cnt[ncnt] == nkeys
        dkey, dline = (_u64 * (nkeys + 1))(), (_u32 * (nkeys + 1))()
        kw, lw = (_u32 * (nkeys + 1))(), (_u32 * (nkeys + 1))()
        assert tsim.lsosim_scatter(value if f else None, cls if f else None, src, sline, nkeys, vmin, vmax, nord, desc, 1, p, cnt,
                                   nkeys, dkey, dline, kw, lw) == 0
        assert list(kw) == [1] * nkeys + [0] and list(lw) == [1] * nkeys + [0]
        src, sline = dkey, dline
    got = list(zip(src, sline))[:nkeys] if passes else []
    assert got == sorted(items), "sorted by (sort key, key number)"
    order = [k for _, k in got]
    assert order == py_order(vals, desc)
    a_keys = (_u32 * max(nkeys, 1))(*order)
    words = tsim.lttsim_index_words(K)
    assert words == 6 + 2 * K
    mask, unset = tsim.lsosim_start_mask(), tsim.lsosim_unset()
    rows = []
    for k in order:
        _, t, fields = lines[st["first"][k]]
        rows.append(bytes([FSEP]).join(b"" if f == "unset" else t[f[0]:f[0] + f[1]] for f in fields) + bytes([DELIM]))
    src_len = (src_off + len(st["buf"]) + 15) // 16 * 16
    source = bytes([0xEE]) * src_off + st["buf"] + bytes([0xEE]) * (src_len - src_off - len(st["buf"]))
    for limit in limits:
        # 4. the ordered table of the rows in front of the limit, into arrays of its own
        nrows = tsim.lttsim_rows(nkeys, limit)
        assert nrows == (min(limit, nkeys) if limit else nkeys)
        nent = nrows * K
        cstart, coff, tw = (_u64 * max(nent, 1))(), (_u64 * (nent + 1))(), (_u32 * max(nent, 1))()
        assert tsim.lttsim_table(a_keys, first, st["a_off"], st["a_start"], nrows, nkeys, n, K, cstart, coff, tw) == 0
        assert list(tw)[:nent] == [1] * nent
        for r in range(nrows):
            e0 = st["first"][order[r]] * K
            for f in range(K):
                assert cstart[r * K + f] == st["start"][e0 + f] and coff[r * K + f] == st["off"][e0 + f + 1] - st["off"][e0 + f] > 0
        tsim.lsosim_scan(coff, nent)
        need = sum(len(t) for t in rows[:nrows])
        assert coff[nent] == need
        for cut in cuts:
            cap = need if cut is None else cut(need, [len(t) for t in rows[:nrows]])
            want, nwritten = b"", 0
            for t in rows[:nrows]:
                if len(want) + len(t) > cap:
                    break
                want += t
                nwritten += 1
            out_bytes = len(want)
            assert out_bytes == coff[nwritten * K]
            if out_bytes:
                # 5. the extract's gather over the ordered table, unchanged
                dst_len = (dst_off + out_bytes + 15) // 16 * 16
                dst = (_u8 * dst_len)(*([FILL] * dst_len))
                reads, writes = (_u32 * max(src_len, 1))(), (_u32 * dst_len)()
                win, glo = _u64(), _u64()
                assert gsim.lesim_gather(coff, cstart, nent, out_bytes, src_off, dst_off, DELIM, FSEP, source, src_len, dst, dst_len,
                                         reads, writes, ctypes.byref(win), ctypes.byref(glo)) == 0
                g, w = bytes(dst), list(writes)
                assert g[dst_off:dst_off + out_bytes] == want
                assert w[dst_off:dst_off + out_bytes] == [1] * out_bytes, "every output byte exactly once"
                assert not any(w[:dst_off]) and not any(w[dst_off + out_bytes:])
            for ccap, scap, icap, rcap in caps:
                # 6. the permute: every word below the caps once, nothing beyond
                crow = nrows if ccap is None else min(ccap, nrows)
                srow = nrows if scap is None else min(scap, nrows)
                irow = nwritten if icap is None else min(icap, nwritten)
                size = nkeys + 3
                oc, ocw = (_u64 * size)(*([7] * size)), (_u32 * size)()
                osum, osw = (_i64 * (4 * V * size))(*([7] * (4 * V * size))), (_u32 * (4 * V * size))()
                idx, iw = (_i64 * (words * size))(*([7] * (words * size))), (_u32 * (words * size))()
                inv, nw = (_u32 * max(nkeys, 1))(), (_u32 * max(nkeys, 1))()
                assert tsim.lttsim_permute(a_keys, nkeys, st["a_counts"], st["a_aggs"], V, first, st["a_ends"], n, cstart, coff, K,
                                           value, cls, oc, crow, ocw, osum, srow, osw, idx, irow, iw, inv, nw) == 0
                assert list(ocw) == [1] * crow + [0] * (size - crow) and list(oc)[crow:] == [7] * (size - crow)
                assert list(oc)[:crow] == [st["counts"][k] for k in order[:crow]]
                assert list(osw) == [1] * (4 * V * srow) + [0] * (4 * V * (size - srow))
                assert list(osum)[:4 * V * srow] == [w_ for k in order[:srow] for c in range(V) for w_ in aggs[k][c]]
                assert list(osum)[4 * V * srow:] == [7] * (4 * V * (size - srow))
                assert list(iw) == [1] * (words * irow) + [0] * (words * (size - irow))
                assert list(idx)[words * irow:] == [7] * (words * (size - irow))
                at = 0
                for r in range(irow):
                    k = order[r]
                    i = st["first"][k]
                    _, t, fields = lines[i]
                    ls = st["ends"][i] - len(t)
                    row = [i, ls, len(t), at]
                    for f in fields:
                        row += [-1, -1] if f == "unset" else [ls + f[0], f[1]]
                    row += [k, vals[k][1] if vals[k][0] else 0]
                    assert list(idx)[words * r:words * (r + 1)] == row, (r, k)
                    at += len(rows[r])
                assert list(nw)[:nkeys] == [1] * nkeys and [inv[k] for k in order] == list(range(nkeys))
                # 7. the ranks of the lines: the inverse of the item order, whatever limit and the caps are
                m = n if rcap is None else min(rcap, n)
                rank, rw = (_i64 * (n + 3))(*([7] * (n + 3))), (_u32 * (n + 3))()
                tsim.lttsim_ranks(st["a_lslot"], st["a_cnt"], inv, m, nkeys, rank, rw)
                assert list(rw) == [1] * m + [0] * (n + 3 - m) and list(rank)[m:] == [7] * (n + 3 - m)
                assert list(rank)[:m] == [-1 if k is None else order.index(k) for k, _, _ in lines[:m]]
    return order, passes


SIZES = (1, 63, 64, 65, 257, 1024 + 17, 2 * 1024 + 1)
# need, need - 1, one row, 0
CUTS = (None, lambda need, rows: need - 1, lambda need, rows: rows[0], lambda need, rows: 0)


@pytest.mark.parametrize("desc", (0, 1), ids=("asc", "desc"))
@pytest.mark.parametrize("by,col", BYS, ids=("count", "sum0", "min0", "max1", "n1", "sum1"))
def test_order(tsim, gsim, by, col, desc):
    for nkeys in SIZES:
        rng = random.Random(nkeys * 100 + by * 10 + desc)
        case = make_case(rng, nkeys)
        tail = nkeys in (65, 1024 + 17)
        run(tsim, gsim, rng, case, by, col, desc, limits=(0, 3) if tail else (0,), src_off=rng.randrange(16), dst_off=rng.randrange(16))


@pytest.mark.parametrize("nkeys", (1, 65, 1024 + 17))
def test_limits_caps_and_cuts(tsim, gsim, nkeys):
    rng = random.Random(nkeys)
    case = make_case(rng, nkeys)
    caps = ((None, None, None, None), (0, 0, 0, 0), (1, 2, 1, 3), (nkeys - 1, nkeys // 2, nkeys - 1, len(case[0]) - 1), (nkeys + 2,) * 4)
    run(tsim, gsim, rng, case, SUM, 1, 1, limits=(0, 1, 3, nkeys, nkeys + 5), caps=caps, cuts=CUTS, src_off=3, dst_off=13)


def test_a_column_without_a_number(tsim, gsim):
    rng = random.Random(4)
    for col1 in ("some", "none"):
        case = make_case(rng, 300, col1=col1)
        for by in (SUM, MIN, MAX):
            for desc in (0, 1):
                order, passes = run(tsim, gsim, rng, case, by, 1, desc)
                bare = [k for k in range(300) if case[1][k][1][3] == 0]
                assert bare and order[len(order) - len(bare):] == bare, "the keys that are not ordered come last, in first-appearance order"
                if col1 == "none":
                    assert order == list(range(300)) and passes == 1
        run(tsim, gsim, rng, case, N, 1, 1)


def test_the_passes_follow_the_range(tsim, gsim):
    rng = random.Random(5)
    case = make_case(rng, 200)
    run(tsim, gsim, rng, case, COUNT, 0, 1, want_passes=1)
    run(tsim, gsim, rng, make_case(rng, 200, big=True), SUM, 0, 0, want_passes=8)
    lines, aggs = case
    for k, a in enumerate(aggs):
        a[0][0] = 300 if k == 7 else k % 100
    run(tsim, gsim, rng, (lines, aggs), SUM, 0, 1, want_passes=2)


def test_the_range_refusal(tsim, gsim):
    assert tsim.lttsim_max_range() == (1 << 64) - 3
    ok = tsim.lttsim_range_ok
    assert ok(2, I64_MIN + 2, I64_MAX) == 1 and ok(2, I64_MIN + 1, I64_MAX) == 0 and ok(2, I64_MIN, I64_MAX) == 0
    assert ok(2, I64_MIN, I64_MAX - 2) == 1 and ok(2, I64_MIN, I64_MAX - 1) == 0
    assert ok(0, I64_MAX, I64_MIN) == 1 and ok(1, I64_MIN, I64_MIN) == 1 and ok(1, I64_MAX, I64_MAX) == 1
    # at the largest range the sort still works: the key of a key that is not ordered is 2^64 - 2, not the reserved word
    rng = random.Random(6)
    lines, aggs = make_case(rng, 70)
    for k, a in enumerate(aggs):
        a[1] = [0, I64_MAX, I64_MIN, 0] if k % 3 == 1 else [rng.randrange(I64_MIN + 2, I64_MAX + 1), 1, 1, 1]
    aggs[0][1][0], aggs[69][1][0] = I64_MAX, I64_MIN + 2
    for desc in (0, 1):
        run(tsim, gsim, rng, (lines, aggs), SUM, 1, desc, want_passes=8)


def test_by_and_by_col(tsim):
    ok = tsim.lttsim_by_ok
    assert [ok(COUNT, 0, v) for v in (0, 1, 8)] == [1, 1, 1] and ok(COUNT, 1, 2) == 0
    for by in (SUM, MIN, MAX, N):
        assert ok(by, 0, 0) == 0 and ok(by, 0, 1) == 1 and ok(by, 1, 1) == 0 and ok(by, 7, 8) == 1 and ok(by, 8, 8) == 0
    assert ok(-1, 0, 1) == 0 and ok(5, 0, 1) == 0
    agg = (_i64 * 4)(-5, -9, 4, 3)
    none = (_i64 * 4)(0, I64_MAX, I64_MIN, 0)
    v = _i64()
    assert [(tsim.lttsim_order(by, 11, agg, ctypes.byref(v)), v.value) for by in (COUNT, SUM, MIN, MAX, N)] == \
        [(1, 11), (1, -5), (1, -9), (1, 4), (1, 3)]
    assert [(tsim.lttsim_order(by, 11, none, ctypes.byref(v)), v.value) for by in (COUNT, SUM, MIN, MAX, N)] == \
        [(1, 11), (-1, 0), (-1, 0), (-1, 0), (1, 0)]
