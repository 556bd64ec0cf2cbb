"""The ordered tally (sre_hip_tally_top_lines): the tally's rows, counts, aggregates and index in the order of the keys'
count or of an aggregate, with a limit, and the rank of every line's key.

Expected values are pure Python over the oracle: the tally-with-sums test's `aggregates` and the tally test's `tally` give
every key's first line, count and aggregates in first-appearance order; the order is `sorted` with key (+-value, k) over the
ordered keys and the others behind.  Every buffer is an Out: 64 guard bytes in front and behind, 0xA5 throughout, and every
check asserts that nothing beyond what the call may write has changed.  A runner asserts of its INPUT that an unordered or
unstable output could not pass: at least two distinct order values, keys not already in output order, and two keys of equal
value with a different one between them in first-appearance order.
"""
import ctypes
import random
import struct

import pytest

import sregex_amd as S
from test_gpu_lines import split_lines, upload_at
from test_gpu_lines_filter import Out, download
from test_gpu_lines_extract import DOTTED, Program, expected, row_text, run_extract
from test_gpu_lines_tally import tally, words
from test_gpu_lines_tally_sums import IDENTITY, INT64_MAX, INT64_MIN, KVW, NINES, OCTETS, aggregates, base6, run_sums
from test_gpu_lines_sort import run_sort

pytestmark = pytest.mark.gpu

COUNT, SUM, MIN, MAX, N = S.HIP_TOP_COUNT, S.HIP_TOP_SUM, S.HIP_TOP_MIN, S.HIP_TOP_MAX, S.HIP_TOP_N
BIG = 10 ** 18 - 1


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def host_passes(max_key):
    return (max(max_key.bit_length(), 1) + 7) // 8


def order_value(by, col, count, aggs):
    """(ordered, value) of a key"""
    if by == COUNT:
        return True, count
    s, lo, hi, n = aggs[col]
    if by == N:
        return True, n
    if n == 0:
        return False, 0
    return True, {SUM: s, MIN: lo, MAX: hi}[by]


def the_order(vals, desc):
    sign = -1 if desc else 1
    return sorted((k for k, (o, _) in enumerate(vals) if o), key=lambda k: (sign * vals[k][1], k)) + [k for k, (o, _) in enumerate(vals) if not o]


def shape_holds(vals, order):
    """an unordered or unstable output could not pass"""
    v = [x for o, x in vals if o]
    if len(set(v)) < 2 or order == list(range(len(vals))):
        return False
    last, between = {}, False
    for i, x in enumerate(v):
        if x in last and any(y != x for y in v[last[x] + 1:i]):
            between = True
            break
        last.setdefault(x, i)
    return between


def run_top(sc, exp, data, groups, vgroups, by=COUNT, col=0, desc=True, limit=0, max_keys=None, delim=0x0A, fsep=0x09, all_lines=False,
            src_off=0, dst_off=0, out_cap=None, counts_cap=None, sums_cap=None, rank_cap=None, index_cap=None, null_out=False,
            overflow=False, refused=False, shape=True):
    """one call, checked in full; returns (info, order, [[count, aggregates ..]] per key in first-appearance order)"""
    lib = sc.lib
    K, V = len(groups), len(vgroups)
    nlines = len(split_lines(data, delim))
    sel = expected(exp, data, delim, groups, all_lines)
    keys, ids = tally(data, sel)
    firsts = [v[0] for v in keys.values()]
    rows_of = list(aggregates(exp, data, delim, groups, vgroups, all_lines).values())
    nkeys = len(keys)
    assert [r[0] for r in rows_of] == [v[1] for v in keys.values()]
    vals = [order_value(by, col, r[0], r[1:]) for r in rows_of]
    order = the_order(vals, desc)
    if shape and nkeys >= 4 and not refused:
        assert shape_holds(vals, order), "the case's input does not exercise the order"
    ordered = [x for o, x in vals if o]
    vmin, vmax = min(ordered, default=INT64_MAX), max(ordered, default=INT64_MIN)
    rng_ = vmax - vmin if ordered else 0
    passes = host_passes(rng_ + 1 if len(ordered) < nkeys else rng_) if nkeys else 0
    nrows = min(limit, nkeys) if limit else nkeys
    texts = [row_text(data, firsts[k][3], fsep, delim) for k in order[:nrows]]
    need = sum(len(t) for t in texts)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for t in texts:
        if out_bytes + len(t) > cap:
            break
        out_bytes += len(t)
        nwritten += 1
    want = b"".join(texts[:nwritten])
    mk = max(nkeys, 1) if max_keys is None else max_keys
    ccap = nkeys + 3 if counts_cap is None else counts_cap
    scap = (nkeys + 3 if V else 0) if sums_cap is None else sums_cap
    rcap = nlines + 3 if rank_cap is None else rank_cap
    icap = nkeys + 3 if index_cap is None else index_cap
    width = 6 + 2 * K
    src = upload_at(data, src_off)
    out, cnt, sums = Out(lib, cap, dst_off), Out(lib, ccap * 8, 0), Out(lib, scap * max(V, 1) * 32, 0)
    rnk, idx = Out(lib, rcap * 8, 0), Out(lib, icap * width * 8, 0)
    try:
        def call():
            return sc.tally_top_lines(src.ptr + src_off, len(data), None if null_out else out.ptr, cap, groups, vgroups, mk, by, col, desc,
                                      limit, delim, fsep, all_lines, cnt.ptr if ccap else None, ccap, sums.ptr if scap else None, scap,
                                      rnk.ptr if rcap else None, rcap, idx.ptr if icap else None, icap)
        if overflow or refused:
            with pytest.raises(S.TallyOverflow if overflow else RuntimeError) as e:
                call()
            if overflow:
                assert e.value.info == S.TallyInfo(nlines, len(sel), 0, 0, 0, 0), e.value.info
            else:
                assert not isinstance(e.value, S.TallyOverflow)
            for o in (out, cnt, sums, rnk, idx):
                o.check(b"")            # 0xA5 throughout
            return None, order, rows_of
        info = call()
        assert info == S.TallyTopInfo(nlines, len(sel), nkeys, len(ordered), nrows, need, nwritten, out_bytes, passes, vmin, vmax), \
            (info, len(sel), nkeys, need, passes)
        out.check(want)
        # counts and aggregates of the rows in front of the limit, whatever out_cap is
        m = min(ccap, nrows)
        assert words(lib, cnt, m, ctypes.c_uint64) == [rows_of[k][0] for k in order[:m]]
        m = min(scap, nrows)
        sums.check(b"".join(struct.pack("<qqqQ", *a) for k in order[:m] for a in rows_of[k][1:]))
        # the rank of every line's key in the FULL order
        inv = {k: r for r, k in enumerate(order)}
        m = min(rcap, nlines)
        assert words(lib, rnk, m) == [inv[ids[i]] if i in ids else -1 for i in range(m)]
        # the index rows of the written rows
        m = min(icap, nwritten)
        rows, o = [], 0
        for k, t in zip(order[:m], texts):
            i, st, n, fields = firsts[k]
            row = [i, st, n, o]
            for f in fields:
                row += list(f) if f else [-1, -1]
            rows.append(tuple(row + [k, vals[k][1] if vals[k][0] else 0]))
            o += len(t)
        raw = words(lib, idx, width * m)
        assert [tuple(raw[width * r:width * (r + 1)]) for r in range(m)] == rows
    finally:
        for b in (src, out, cnt, sums, rnk, idx):
            b.free()
    return info, order, rows_of


def top_lines(seed, nkeys, extra=2.0, span=6, miss=0.1, heavy=0, big=False):
    """lines k=KEY;v=NUMBER;w=TEXT; of under 100 bytes over exactly nkeys distinct keys, every key on one line at least;
    w holds a number on no line of every third key and on some lines of the others; some lines have no match"""
    rng = random.Random(seed)
    keys = [base6(j + 1) for j in range(nkeys)]
    picks = list(range(nkeys)) + [rng.randrange(nkeys) for _ in range(int(extra * nkeys))] + [nkeys // 2] * heavy
    rng.shuffle(picks)
    pads = [b"", b" ", b"-- ", b"at 12 "]
    out = []
    for i, j in enumerate(picks):
        if rng.random() < miss:
            out.append(b"no key here;v=1;")
        v = rng.randrange(-BIG, BIG + 1) if big else rng.randrange(-span, span)
        w = b"%d" % rng.randrange(-span, span) if j % 3 != 1 and rng.random() < 0.7 else rng.choice((b"", b"x1", b"-"))
        out.append(pads[i % 4] + b"k=" + keys[j] + b";v=%d;w=" % v + w + b";" + pads[(i // 4) % 4])
    assert max(len(t) for t in out) < 100
    return b"\n".join(out) + (b"\n" if nkeys % 2 else b"")


BYS = [(COUNT, 0), (SUM, 0), (MIN, 0), (MAX, 0), (N, 1), (SUM, 1)]
BY_IDS = ["count", "sum0", "min0", "max0", "n1", "sum1"]


# ------------------------------------------------------------------ 1. sizes, orders, directions, limits

@pytest.mark.parametrize("nkeys", [1, 63, 64, 65, 257, 1024 + 17, 2 * 1024 + 1])
def test_key_counts_at_the_slot_and_workgroup_edges(gpu, nkeys):
    data = top_lines(nkeys, nkeys, extra=1.5 if nkeys > 1000 else 2.5)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        for (by, col), desc in zip(BYS, (True, False, True, False, True, False)):
            info, _, _ = run_top(p.sc, p.exp, data, [1], [2, 3], by, col, desc, src_off=nkeys % 16, dst_off=(3 * nkeys) % 16)
            assert info.nkeys == nkeys and p.sc.last_lines_device == 1


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("by,col", BYS, ids=BY_IDS)
def test_every_order_both_directions_and_the_limits(gpu, by, col, desc):
    data = top_lines(7, 90)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        for limit in (0, 1, 3, 90, 95):
            info, _, _ = run_top(p.sc, p.exp, data, [1, 2] if limit == 3 else [1], [2, 3], by, col, desc, limit=limit)
            assert info.nrows == (min(limit, info.nkeys) if limit else info.nkeys)


def test_the_passes_follow_the_range(gpu):
    with S.Pool() as pool:
        p = Program(pool, KVW)
        info, _, _ = run_top(p.sc, p.exp, top_lines(1, 70), [1], [2, 3], COUNT)
        assert info.passes == 1 and info.vmax <= 255
        info, order, rows = run_top(p.sc, p.exp, top_lines(2, 70, heavy=300), [1], [2, 3], COUNT)
        assert info.passes == 2 and info.vmax > 300 and rows[order[0]][0] == info.vmax
        info, _, _ = run_top(p.sc, p.exp, top_lines(3, 70, big=True), [1], [2], SUM, 0, shape=False)
        assert info.passes == 8
        info, _, _ = run_top(p.sc, p.exp, top_lines(3, 70, big=True), [1], [2], SUM, 0, desc=False, shape=False)
        assert info.passes == 8


def test_a_column_without_a_number_for_some_keys_and_for_all(gpu):
    data = top_lines(4, 80)
    none = b"\n".join(b"k=%s;v=x%d;w=;" % (base6(1 + i % 11), i) for i in range(60))
    with S.Pool() as pool:
        p = Program(pool, KVW)
        for by in (SUM, MIN, MAX):
            for desc in (False, True):
                info, order, rows = run_top(p.sc, p.exp, data, [1], [2, 3], by, 1, desc)
                bare = [k for k, r in enumerate(rows) if r[2][3] == 0]
                assert 20 < len(bare) < 60 and order[-len(bare):] == bare and info.nordered == 80 - len(bare)
                info, order, _ = run_top(p.sc, p.exp, none, [1], [2, 3], by, 0, desc, shape=False)
                assert info.nordered == 0 and order == list(range(11)) and info.passes == 1
                assert (info.vmin, info.vmax) == (INT64_MAX, INT64_MIN)
        info, _, _ = run_top(p.sc, p.exp, none, [1], [2, 3], N, 0, shape=False)
        assert info.nordered == 11 and (info.vmin, info.vmax) == (0, 0)


def test_a_wrapping_sum_is_ordered_as_stored(gpu):
    lines = [b"k=p;v=" + NINES + b";w=;"] * 12 + [b"k=m;v=-" + NINES + b";w=;"] * 12 + [b"k=z;v=5;w=;", b"k=y;v=-5;w=;", b"k=q;v=5;w=;"]
    random.Random(5).shuffle(lines)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        info, order, rows = run_top(p.sc, p.exp, b"\n".join(lines), [1], [2], SUM, 0, True, shape=False)
        stored = [r[1][0] for r in rows]
        assert 12 * BIG - (1 << 64) in stored and (1 << 64) - 12 * BIG in stored
        assert [stored[k] for k in order] == sorted(stored, reverse=True) and stored[order[0]] == (1 << 64) - 12 * BIG
        assert info.passes == 8


def test_the_range_refusal(gpu):
    """sums of exactly INT64_MAX and INT64_MIN: vmax - vmin is 2^64 - 1, beyond the 2^64 - 3 the sort's keys hold; one step
    inside (INT64_MIN + 2 .. INT64_MAX: exactly 2^64 - 3) the call sorts"""
    def summing_to(key, total):
        sign, rest, out = (b"-", -total, []) if total < 0 else (b"", total, [])
        while rest > 0:
            x = min(rest, BIG)
            out.append(b"k=" + key + b";v=" + sign + b"%d" % x + b";w=;")
            rest -= x
        return out
    hi, lo = summing_to(b"hi", INT64_MAX), summing_to(b"lo", INT64_MIN)
    assert 18 <= len(hi) + len(lo) <= 22
    with S.Pool() as pool:
        p = Program(pool, KVW)
        for desc in (False, True):
            lines = hi + lo + [b"k=bare;v=;w=;", b"k=mid;v=7;w=;"]
            random.Random(9).shuffle(lines)
            run_top(p.sc, p.exp, b"\n".join(lines), [1], [2], SUM, 0, desc, refused=True)
            # the other orders of the same buffer are in range
            run_top(p.sc, p.exp, b"\n".join(lines), [1], [2], COUNT, 0, desc, shape=False)
            inside = hi + summing_to(b"lo", INT64_MIN + 2) + [b"k=bare;v=;w=;", b"k=mid;v=7;w=;"]
            random.Random(9).shuffle(inside)
            info, order, rows = run_top(p.sc, p.exp, b"\n".join(inside), [1], [2], SUM, 0, desc, shape=False)
            assert info.vmax - info.vmin == (1 << 64) - 3 and info.passes == 8 and info.nordered == 3
            assert rows[order[-1]][1] == IDENTITY


def test_all_lines_and_the_all_empty_key(gpu):
    data = top_lines(5, 70, miss=0.3)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        info, order, rows = run_top(p.sc, p.exp, data, [1], [2, 3], COUNT, all_lines=True)
        assert info.nselected == info.nlines and info.nkeys == 71
        empty = next(k for k, r in enumerate(rows) if r[0] > 10)
        assert order[0] == empty, "the lines without a match carry the all-empty key, the heaviest here"
        run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 1, False, all_lines=True)
        run_top(p.sc, p.exp, b"", [1], [2, 3], COUNT, all_lines=True)
        info, _, _ = run_top(p.sc, p.exp, b"nothing\nat all\n", [1], [2, 3], MAX, 0, all_lines=True)
        assert info.nkeys == 1 and info.nordered == 0
        info, _, _ = run_top(p.sc, p.exp, b"nothing\nat all\n", [1], [2, 3], MAX, 0)
        assert info == S.TallyTopInfo(2, 0, 0, 0, 0, 0, 0, 0, 0, INT64_MAX, INT64_MIN)


def test_the_count_order_without_value_groups(gpu):
    data = top_lines(6, 80)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        run_top(p.sc, p.exp, data, [1], [], COUNT)
        run_top(p.sc, p.exp, data, [1], [], COUNT, desc=False, limit=5)
        # with value groups the count order needs no sums either
        run_top(p.sc, p.exp, data, [1], [2, 3], COUNT, sums_cap=0)


# ------------------------------------------------------------------ 2. capacities, alignment, overflow

def test_the_sizing_call_the_cut_and_every_cap(gpu):
    data = top_lines(8, 70)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        info, order, _ = run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0)
        nkeys, need, nlines = info.nkeys, info.need_bytes, info.nlines
        got, _, _ = run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, out_cap=0, null_out=True)
        assert got.need_bytes == need and got.nwritten == 0 and got.nrows == nkeys
        row = run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, limit=1)[0].need_bytes       # the first row's bytes
        for cap in (need, need - 1, row, row - 1, 0):
            got, _, _ = run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, out_cap=cap, dst_off=3)
            assert got.nwritten == {need: nkeys, need - 1: nkeys - 1, row: 1, row - 1: 0, 0: 0}[cap] and got.need_bytes == need
        for limit in (0, 10):
            for ccap, scap, rcap, icap in ((0, 0, 0, 0), (5, 3, 17, 2), (nkeys, 1, nlines, 9), (1, nkeys + 2, nlines - 1, nkeys), (9, 10, 1, 11)):
                run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, limit=limit, counts_cap=ccap, sums_cap=scap, rank_cap=rcap, index_cap=icap)
            # the index stops at the rows written, the counts and the aggregates do not
            whole, _, _ = run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, limit=limit)
            got, _, _ = run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, limit=limit, out_cap=whole.need_bytes // 3)
            assert 0 < got.nwritten < got.nrows == whole.nrows


@pytest.mark.parametrize("src_off", [1, 7, 13, 15])
def test_odd_alignments(gpu, src_off):
    data = top_lines(src_off, 120).rstrip(b"\n -")
    with S.Pool() as pool:
        p = Program(pool, KVW)
        run_top(p.sc, p.exp, data, [1, 2], [2, 3], MIN, 0, src_off % 2 == 1, src_off=src_off, dst_off=16 - src_off)
        run_top(p.sc, p.exp, data, [1], [3], N, 0, True, limit=7, src_off=src_off, dst_off=(src_off * 5) % 16)


def test_overflow_writes_nothing(gpu):
    data = top_lines(9, 66)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, max_keys=65, overflow=True)
        run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, max_keys=66)
        run_top(p.sc, p.exp, data, [1], [2, 3], COUNT, max_keys=1, overflow=True, limit=3)


# ------------------------------------------------------------------ 3. batches and the other routes

def test_a_keys_lines_fall_into_different_batches(gpu, monkeypatch):
    data = top_lines(11, 12, extra=7.0)
    with S.Pool() as pool:
        p = Program(pool, KVW)
        _, one, rows = run_top(p.sc, p.exp, data, [1], [2, 3], MIN, 0, src_off=1, dst_off=2)
        assert p.sc.last_line_batches == 1
        assert max(r[0] for r in rows) > 7, "a key with more lines than a batch of 7 holds"
        monkeypatch.setenv("SRE_HIP_LINES_BATCH", "7")
        _, two, _ = run_top(p.sc, p.exp, data, [1], [2, 3], MIN, 0, src_off=1, dst_off=2)
        assert p.sc.last_line_batches > 10 and one == two


def dotted_lines(seed, nlines=600):
    rng = random.Random(seed)
    addrs = [b"%d.%d.%d.%d" % (rng.randrange(4), rng.randrange(256), rng.randrange(256), rng.randrange(256)) for _ in range(60)]
    return b"\n".join(rng.choice([b"GET / from ", b"", b"x "]) + rng.choice(addrs + [b"1.2.3", b"none"]) + b" ok" for _ in range(nlines))


@pytest.mark.parametrize("pats,groups,vgroups,by", [(DOTTED, [0], [1, 0], COUNT), (OCTETS, [2], [1, 2], SUM)], ids=["dotted", "octets"])
def test_a_counted_repeat_on_the_nfa_tier_and_its_host_route(gpu, monkeypatch, pats, groups, vgroups, by):
    data = dotted_lines(2)
    with S.Pool() as pool:
        p = Program(pool, pats, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        info, one, _ = run_top(p.sc, p.exp, data, groups, vgroups, by, 0, src_off=3, dst_off=5)
        assert p.sc.last_lines_device == 1 and info.nselected < info.nlines and info.nkeys > 40
        monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
        _, two, _ = run_top(p.sc, p.exp, data, groups, vgroups, by, 0, src_off=3, dst_off=5)
        assert p.sc.last_lines_device == 0 and one == two


def test_thompson_and_count_scanners_are_refused(gpu):
    data = b"k=a;v=1;w=2;\n"
    src, out = upload_at(data, 0), Out(gpu, 64, 0)
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, KVW))
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                with pytest.raises(RuntimeError):
                    S.Scanner(pool, prog, mode).tally_top_lines(src.ptr, len(data), out.ptr, 64, [1], [2], 4)
            out.check(b"")
    finally:
        src.free()
        out.free()


# ------------------------------------------------------------------ 4. the output as a dictionary, the scanner's other calls

def test_the_output_is_a_dictionary_whose_ids_are_the_ranks(gpu):
    data = top_lines(12, 150, miss=0.2)
    nlines = len(split_lines(data, 0x0A))
    src = upload_at(data, 0)
    out, rnk, kid, cnt = Out(gpu, len(data), 0), Out(gpu, nlines * 8, 0), Out(gpu, nlines * 8, 0), Out(gpu, 150 * 8, 0)
    routed = Out(gpu, len(data) + 1, 0)
    try:
        with S.Pool() as pool:
            p = Program(pool, KVW)
            info = p.sc.tally_top_lines(src.ptr, len(data), out.ptr, len(data), [1], [2], 150, COUNT, 0, True, counts_ptr=cnt.ptr,
                                        counts_cap=150, rank_ptr=rnk.ptr, rank_cap=nlines)
            assert info.nkeys == info.nwritten == 150
            ranks = words(gpu, rnk, nlines)
            counts = words(gpu, cnt, 150, ctypes.c_uint64)
            assert counts == sorted(counts, reverse=True) and counts[0] > counts[-1]
            ks = S.KeySet(out.ptr, info.out_bytes, 1, lib=gpu)
            try:
                assert ks.rows == 150 and ks.distinct == 150
                p.sc.lookup_lines(src.ptr, len(data), None, 0, [1], ks, keyid_ptr=kid.ptr, keyid_cap=nlines)
                ids = words(gpu, kid, nlines)
                assert [-1 if v == -2 else v for v in ids] == ranks and -1 in ranks and set(ranks) >= set(range(150))
                got = p.sc.route_lines_by_key(src.ptr, len(data), routed.ptr, len(data) + 1, [1], ks)
                text = download(gpu, routed.ptr, got.out_bytes).split(b"\n")
                heaviest = download(gpu, out.ptr, info.out_bytes).split(b"\n")[0]
                head = text[:counts[0]]
                assert all(b"k=" + heaviest + b";" in t for t in head) and b"k=" + heaviest + b";" not in text[counts[0]]
            finally:
                ks.close()
    finally:
        for b in (src, out, rnk, kid, cnt, routed):
            b.free()


def test_the_scanners_other_calls_behave_as_on_a_fresh_scanner(gpu):
    data = top_lines(13, 60)
    with S.Pool() as pool:
        p, fresh = Program(pool, KVW), Program(pool, KVW)
        _, want_rows, _ = run_extract(fresh.sc, fresh.exp, data, [1, 2], src_off=2, dst_off=9)
        _, want_sums = run_sums(fresh.sc, fresh.exp, data, [1], [2, 3], src_off=2, dst_off=9)
        want_sort = run_sort(fresh.sc, fresh.exp, data, 2, desc=True, src_off=2, dst_off=9)
        run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, src_off=2, dst_off=9)
        run_top(p.sc, p.exp, data, [1, 2], [3], COUNT, max_keys=3, overflow=True)
        _, got_sums = run_sums(p.sc, p.exp, data, [1], [2, 3], src_off=2, dst_off=9)
        got_sort = run_sort(p.sc, p.exp, data, 2, desc=True, src_off=2, dst_off=9)
        _, got_rows, _ = run_extract(p.sc, p.exp, data, [1, 2], src_off=2, dst_off=9)
        assert got_sums == want_sums and got_sort == want_sort and got_rows == want_rows
        run_top(p.sc, p.exp, data, [1], [3, 2], MAX, 1, False, limit=4, src_off=2, dst_off=9)


def test_scratch_that_grows_inside_a_call_on_a_used_scanner(gpu):
    """a scanner whose arrays are sized for 60 lines takes 2 101 lines over 1 025 keys: two workgroups of the values pass, three
    blocks of the entry table's scan, two digit passes; every array of the ordered tally grows inside that call, and the sort
    and the tally with sums behind it find what a fresh scanner finds"""
    small, data = top_lines(14, 20, miss=0), top_lines(15, 1025, extra=1.05, span=300, miss=0)
    assert len(split_lines(small, 0x0A)) == 60 and len(split_lines(data, 0x0A)) == 2101
    with S.Pool() as pool:
        p, fresh = Program(pool, KVW), Program(pool, KVW)
        want_top, _, _ = run_top(fresh.sc, fresh.exp, data, [1], [2, 3], SUM, 0, src_off=2, dst_off=9)
        assert want_top.nkeys == 1025 and want_top.vmax - want_top.vmin >= 256 and want_top.passes >= 2
        want_sort = run_sort(fresh.sc, fresh.exp, data, 2, desc=True, src_off=2, dst_off=9)
        want_sums, _ = run_sums(fresh.sc, fresh.exp, data, [1], [2, 3], src_off=2, dst_off=9)
        run_top(p.sc, p.exp, small, [1], [2, 3], SUM, 0)
        got_top, _, _ = run_top(p.sc, p.exp, data, [1], [2, 3], SUM, 0, src_off=2, dst_off=9)
        got_sort = run_sort(p.sc, p.exp, data, 2, desc=True, src_off=2, dst_off=9)
        got_sums, _ = run_sums(p.sc, p.exp, data, [1], [2, 3], src_off=2, dst_off=9)
        assert got_top == want_top and got_sort == want_sort and got_sums == want_sums
