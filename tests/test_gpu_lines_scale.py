"""Line mode and the line sinks at the sizes the product is built for: entry tables beyond 2^20 entries, calls that
cross the default batch of 2^20 lines, and batches that the device cuts short.

Four paths, each proved reached by assertions on Python-side counts and on the scanner's diagnostics:

1. the one-workgroup scan of the block sums (sre_k_filter_scan) with more than one block per lane, and what reads
   its result behind block 1023: the finish kernels, the gather and the index.  A lane scans per = ceil(blocks /
   LANES) blocks, a block holds ITEMS entries: per >= 2 needs more than LANES * ITEMS = 2^20 entries in one call.
2. a sink call and scan_lines across the default batch BATCH = 2^20 lines: i0 > 0 with many workgroups in a batch,
   for the select passes, the compaction and the NFA tier's short-line kernel.
3. a batch that sre_k_lines_plan ends early because the capture scratch does not fit: (lines of the batch) *
   (segment + 16) * 2 <= WALK_MAX.  With a fixed segment of 2^18 bytes a batch has 2047 lines: odd batch starts,
   two workgroups a batch, a select pass launched for more lines than the batch has.
4. (in test_gpu_lines_extract.py and test_gpu_lines_subst.py: the per-line host route with several batches)

The constants below are the library's; a change of SRE_LINES_BATCH, SRE_LINES_ITEMS, the lanes of sre_k_filter_scan
or the scratch rule of sre_k_lines_plan means these tests no longer reach their paths: their shape assertions fail
and point here.

Not tested: the NFA tier's own scratch cut (sre_k_lines_plan_nfa).  A segment costs it tens of bytes against a
limit of 1 GiB, so it takes tens of millions of lines.

Every expected value comes from the oracle's first-match record of a line and Python slicing, by the rules of
test_gpu_lines_filter.py, test_gpu_lines_extract.py and test_gpu_lines_subst.py (their `expected`, applied once per
distinct line content); the lines of a buffer are drawn from a small pool, so the oracle runs a few hundred times.
Where the helpers of those files would build a Python tuple per row and field, `bulk_run` beside them compares the
same things as numpy arrays; test_the_bulk_path_agrees_with_the_helpers holds it to them.
"""
import functools
import random

import numpy as np
import pytest

import sregex_amd as S
from test_gpu_lines import Expect, check, split_lines, upload_at
from test_gpu_lines_filter import Out, download, run_filter
from test_gpu_lines_filter import expected as filter_expected
from test_gpu_lines_extract import DOTTED, URI, WORDS, row_text, run_extract
from test_gpu_lines_extract import expected as extract_expected
from test_gpu_lines_subst import max_group, pieces_of, run_subst
from test_gpu_lines_subst import expected as subst_expected

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
# sre_hip_lines.h: SRE_LINES_BATCH lines a batch, SRE_LINES_ITEMS entries a block of the sums, SRE_LINES_WALK_MAX
# bytes of capture scratch a batch; sre_hip_lines_gather.hip: sre_k_filter_scan is one workgroup of 1024 lanes
BATCH = 1 << 20
ITEMS = 1024
LANES = 1024
WALK_MAX = 1 << 30


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def blocks_of(nentries):
    return (nentries + ITEMS - 1) // ITEMS


def per_lane(nentries):
    """block sums a lane of sre_k_filter_scan takes"""
    return (blocks_of(nentries) + LANES - 1) // LANES


# ------------------------------------------------------------------ buffers and expectations as arrays

class Lines:
    """a buffer of the lines pool[cid[0]], pool[cid[1]], ... without a final delimiter; the line table comes from
    split_lines"""

    def __init__(self, pool, cid, delim=0x0A):
        assert len(set(pool)) == len(pool) <= 400 and b"" in pool
        assert pool[cid[-1]] != b""         # (an empty last line would be none: the buffer would end with the delimiter)
        self.pool, self.delim = pool, delim
        self.cid = np.asarray(cid, dtype=np.int64)
        self.data = bytes([delim]).join([pool[c] for c in cid])
        table = np.array(split_lines(self.data, delim), dtype=np.int64)
        self.n = len(cid)
        assert table.shape == (self.n, 2)
        self.start, self.len = table[:, 0].copy(), table[:, 1].copy()
        assert np.array_equal(self.len, np.array([len(p) for p in pool], dtype=np.int64)[self.cid])

    def head(self, n):
        """the first n lines as a buffer of their own"""
        cid = self.cid[:n].copy()
        if self.pool[cid[-1]] == b"":
            cid[-1] = next(c for c, p in enumerate(self.pool) if p)
        return Lines(self.pool, cid, self.delim)


LIT, START, ROW = 0, 1, 2       # an index word is a value, or a value + the line's start, or + the row's output offset


def filter_tables(exp, pool, delim, mode):
    """per content: selected without INVERT?, the row's text, no index words behind the first four"""
    d = bytes([delim])
    hit = []
    for line in pool:
        hit.append(len(filter_expected(exp, line + d, delim, mode)) == 1)
    return np.array(hit), [line + d for line in pool], None, None


def extract_tables(exp, pool, delim, groups, fsep=0x09):
    hit, text, val, base = [], [], [], []
    for line in pool:
        [(_, _, _, fields)] = extract_expected(exp, line + bytes([delim]), delim, groups, True)
        hit.append(len(extract_expected(exp, line + bytes([delim]), delim, groups, False)) == 1)
        text.append(row_text(line, fields, fsep, delim))
        val.append([x for f in fields for x in (f if f else (-1, -1))])
        base.append([x for f in fields for x in ((START, LIT) if f else (LIT, LIT))])
    return np.array(hit), text, val, base


def subst_tables(exp, pool, delim, template, ncaps):
    pieces = pieces_of(template, ncaps)
    hit, text, val, base = [], [], [], []
    for line in pool:
        [(_, _, _, m, row)] = subst_expected(exp, line + bytes([delim]), delim, pieces, True)
        hit.append(m is not None)
        text.append(row + bytes([delim]))
        val.append([m[0], m[1], m[0], m[2]] if m else [-1] * 4)
        base.append([START, LIT, ROW, LIT] if m else [LIT] * 4)
    return np.array(hit), text, val, base


class Plan:
    """what one sink call over a Lines buffer has to produce, from the per-content tables: the selected lines, the
    whole output, the end of every row in it and every index row"""

    def __init__(self, buf, tables, invert=False, all_lines=False):
        hit, text, val, base = tables
        select = np.ones(buf.n, dtype=bool) if all_lines else hit[buf.cid] != invert
        self.nlines = buf.n
        self.lines = np.nonzero(select)[0]
        cid = buf.cid[self.lines]
        self.sizes = np.array([len(t) for t in text], dtype=np.int64)[cid]
        assert (self.sizes > 0).all()
        self.ends = np.cumsum(self.sizes)
        self.need = int(self.ends[-1]) if len(cid) else 0
        self.full = b"".join([text[c] for c in cid.tolist()])
        assert len(self.full) == self.need
        offs = self.ends - self.sizes
        start = buf.start[self.lines]
        index = np.stack([self.lines, start, buf.len[self.lines], offs], axis=1)
        if val is not None:
            v, b = np.array(val, dtype=np.int64)[cid], np.array(base, dtype=np.int64)[cid]
            tail = v + np.where(b == START, start[:, None], 0) + np.where(b == ROW, offs[:, None], 0)
            index = np.concatenate([index, tail], axis=1)
        self.index = np.ascontiguousarray(index, dtype=np.int64)

    def cut(self, cap):
        """(rows that fit cap whole, their bytes): the rows take a byte each at least, so their ends ascend strictly"""
        k = int(np.searchsorted(self.ends, cap, side="right"))
        return k, int(self.ends[k - 1]) if k else 0

    def rows_in_front_of(self, line):
        return int(np.searchsorted(self.lines, line, side="left"))


def bulk_run(lib, plan, src, data, call, out_cap=None, index_cap=None, dst_off=5):
    """one sink call checked as run_filter / run_extract / run_subst check theirs: info, output, both guards, the
    source unchanged, the index rows and nothing behind them.  call(out_ptr, out_cap, index_ptr, index_cap)"""
    width = plan.index.shape[1]
    cap = plan.need + 37 if out_cap is None else int(out_cap)
    nwritten, out_bytes = plan.cut(cap)
    icap = len(plan.lines) + 3 if index_cap is None else index_cap
    out = Out(lib, cap, dst_off)
    idx = Out(lib, icap * width * 8, 0)
    try:
        info = call(out.ptr, cap, idx.ptr if icap else None, icap)
        assert info == S.FilterInfo(plan.nlines, len(plan.lines), plan.need, nwritten, out_bytes), (info, len(plan.lines), plan.need)
        out.check(plan.full[:out_bytes])
        assert download(lib, src, len(data)) == data
        nrows = min(icap, nwritten)
        raw = download(lib, idx.ptr, 8 * width * nrows)
        got, want = np.frombuffer(raw, dtype=np.int64).reshape(nrows, width), plan.index[:nrows]
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).any(axis=1))[0][:3]
            raise AssertionError([(int(r), got[r].tolist(), want[r].tolist()) for r in bad])
        idx.check(raw)                  # nothing behind the rows, nothing around the index
    finally:
        out.free()
        idx.free()
    return info


def filter_call(sc, src, n, delim=0x0A, invert=False, all_lines=False):
    return lambda o, cap, i, icap: sc.filter_lines(src, n, o, cap, delim, invert, all_lines, i, icap)


def extract_call(sc, src, n, groups, delim=0x0A, all_lines=False):
    return lambda o, cap, i, icap: sc.extract_lines(src, n, groups, o, cap, delim, 0x09, all_lines, i, icap)


def subst_call(sc, src, n, template, delim=0x0A, all_lines=False):
    return lambda o, cap, i, icap: sc.substitute_lines(src, n, template, o, cap, delim, all_lines, i, icap)


def program(pool, pats):
    re = S.parse(pool, pats)
    prog = S.compile(pool, re)
    return prog, re.ncaps, Expect(prog, re.ncaps, key=("scale", tuple(pats)))


# ------------------------------------------------------------------ 1. tables over 2^21 entries in one batch

DIGIT = [rb"k=(\d)(x*)(y)?"]            # group 2 is set and may be empty, group 3 is set or unset
HITS = [b"k=1", b"k=2x", b"k=3xxy", b"ak=4y", b"k=5 k=6x", b"k=7xx", b"=k=8", b"k=9y"]
MISSES = [b"", b"k=z", b"k=", b"x", b"zz", b"k 1"]
K32 = [0, 1, 2, 3] * 8
T30 = b"$1x" * 13 + b"$2-$3;"          # 30 pieces: 32 entries a line
NTABLE, NSMALL = 66000, 33100
RUN0, RUN = 40000, 3500                 # a run of lines without a match: whole blocks of zero entries


@functools.lru_cache(maxsize=None)
def table_lines(nlines):
    """66000 lines of a few bytes, two in three match, in a seeded random order; the lines RUN0 .. RUN0 + RUN do not
    match; the first `nlines` of them"""
    rng = random.Random(66)
    nh, nm = len(HITS), len(MISSES)
    cid = [rng.randrange(nh) if rng.random() < 2 / 3 else nh + rng.randrange(nm) for _ in range(NTABLE)]
    for i in range(RUN0, RUN0 + RUN):
        cid[i] = nh + rng.randrange(nm)
    for last in (NSMALL, NTABLE):       # the last line of either shape matches (and is not empty)
        for i in range(last - 3, last):
            cid[i] = rng.randrange(nh)
    return Lines(HITS + MISSES, cid[:nlines])


def table_shape(buf, tables, entries, all_lines):
    """the plan of a call over a table of `entries` entries a line, and the cuts [(rows in front, block of the
    boundary entry)] in the blocks 1024, 1025, 1026 (the three places in a lane's run of three) and the last one"""
    plan = Plan(buf, tables, all_lines=all_lines)
    nblk = blocks_of(buf.n * entries)
    cuts = []
    for block in (1024, 1025, 1026, nblk - 1):
        k = plan.rows_in_front_of(block * ITEMS // entries + 5)
        line = int(plan.lines[k])               # the first line that is not written: its first entry is the boundary
        assert line * entries // ITEMS == block, (line, block)
        cuts.append((k, block))
    return plan, cuts


def check_table_shape(buf, hit):
    assert buf.n * 32 == 2112000 and blocks_of(buf.n * 32) == 2063 and per_lane(buf.n * 32) == 3
    assert (2063 - 1) // 3 == 687 and 2063 - 687 * 3 == 2      # the last active lane scans two blocks
    assert list(hit) == [True] * len(HITS) + [False] * len(MISSES)
    miss = ~hit[buf.cid]
    assert 0.3 < miss.mean() < 0.4
    assert miss[RUN0:RUN0 + RUN].all() and RUN >= 3000 and RUN0 * 32 > LANES * ITEMS
    assert RUN * 32 // ITEMS > 100                              # a hundred blocks whose sums are zero


def run_cuts(gpu, plan, cuts, src, data, call):
    for k, _ in cuts:
        for cap in (plan.ends[k - 1], plan.ends[k] - 1):
            info = bulk_run(gpu, plan, src, data, call, out_cap=cap, index_cap=5)
            assert info.nwritten == k and info.out_bytes == plan.ends[k - 1] and info.nselected == len(plan.lines)
            assert plan.full[:info.out_bytes].endswith(b"\n")


def test_extract_over_2_21_entries(gpu):
    buf = table_lines(NTABLE)
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, DIGIT)
        tables = extract_tables(exp, buf.pool, 0x0A, K32)
        check_table_shape(buf, tables[0])
        words = [w for row in tables[2][:len(HITS)] for w in row]
        assert -1 in words and 0 in words[1::2] and 1 in words[1::2]        # unset, empty and set fields
        assert max(len(t) for t in tables[1]) < 128                         # 16 KiB of output: thousands of entries
        shapes = {all_lines: table_shape(buf, tables, 32, all_lines) for all_lines in (False, True)}
        for plan, _ in shapes.values():
            assert int(plan.lines[39999]) * 32 > LANES * ITEMS              # the index rows reach beyond entry 2^20
        sc = S.Scanner(pool, prog, FIRST)
        assert sc.engine == S.ENGINE_SCAN
        src = upload_at(buf.data, 3)
        try:
            for all_lines, (plan, cuts) in shapes.items():
                call = extract_call(sc, src.ptr + 3, len(buf.data), K32, all_lines=all_lines)
                bulk_run(gpu, plan, src.ptr + 3, buf.data, call, index_cap=40000)
                assert sc.last_line_batches == 1 and sc.last_lines_device == 1
                if not all_lines:
                    run_cuts(gpu, plan, cuts, src.ptr + 3, buf.data, call)
        finally:
            src.free()


@pytest.mark.parametrize("all_lines", [False, True], ids=["matching", "all"])
def test_substitute_over_2_21_entries(gpu, all_lines):
    buf = table_lines(NTABLE)
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, DIGIT)
        tables = subst_tables(exp, buf.pool, 0x0A, T30, ncaps)
        assert len(pieces_of(T30, ncaps)) == 30
        check_table_shape(buf, tables[0])
        plan, cuts = table_shape(buf, tables, 32, all_lines)
        sc = S.Scanner(pool, prog, FIRST)
        assert sc.engine == S.ENGINE_SCAN and max_group(sc) == ncaps
        src = upload_at(buf.data, 3)
        try:
            call = subst_call(sc, src.ptr + 3, len(buf.data), T30, all_lines=all_lines)
            bulk_run(gpu, plan, src.ptr + 3, buf.data, call)                # the whole index, 8 words a row
            assert sc.last_line_batches == 1 and sc.last_lines_device == 1
            run_cuts(gpu, plan, cuts, src.ptr + 3, buf.data, call)
        finally:
            src.free()


def test_extract_two_blocks_a_lane(gpu):
    """33100 lines x 32 entries are 1035 blocks: the lanes 0 .. 516 scan two, lane 517 one, the others none"""
    buf = table_lines(NSMALL)
    assert blocks_of(buf.n * 32) == 1035 and per_lane(buf.n * 32) == 2 and (1035 + 1) // 2 == 518
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, DIGIT)
        tables = extract_tables(exp, buf.pool, 0x0A, K32)
        plan = Plan(buf, tables)
        sc = S.Scanner(pool, prog, FIRST)
        assert sc.engine == S.ENGINE_SCAN
        src = upload_at(buf.data, 3)
        try:
            call = extract_call(sc, src.ptr + 3, len(buf.data), K32)
            bulk_run(gpu, plan, src.ptr + 3, buf.data, call)
            assert sc.last_line_batches == 1 and sc.last_lines_device == 1
            cuts = []
            for block in (1024, 1025, 1034):
                k = plan.rows_in_front_of(block * ITEMS // 32 + 5)
                assert int(plan.lines[k]) * 32 // ITEMS == block
                cuts.append((k, block))
            run_cuts(gpu, plan, cuts, src.ptr + 3, buf.data, call)
        finally:
            src.free()


# ------------------------------------------------------------------ 2. more than 2^20 lines, the default batch

NMANY = BATCH + 1500
K_LINES = [b"k=1", b"k=2x", b"ab k=3xxy", b"k=4y k=5", b" k=6xx@"]
DOTTED_LINES = [b"1.2.3.4", b"10.0.0.255", b"x1.22.3.4.", b"a 9.9.9.99", b"255.1.1.1@"]


@functools.lru_cache(maxsize=None)
def many_lines():
    """2^20 + 1500 lines of 0 .. 12 bytes from a pool of 200: five contents match DIGIT, five others DOTTED"""
    rng = random.Random(2020)
    pool = [b""] + K_LINES + DOTTED_LINES
    while len(pool) < 200:
        line = bytes(rng.choice(b"ab c.@x-") for _ in range(rng.randrange(1, 13)))
        if line not in pool:
            pool.append(line)
    cid = [rng.randrange(200) for _ in range(NMANY)]
    cid[-1] = 1
    buf = Lines(pool, cid)
    assert buf.n == NMANY and blocks_of(buf.n) == 1026 and per_lane(buf.n) == 2
    assert int(buf.len.max()) == 12 and 6 << 20 < len(buf.data) < 9 << 20
    return buf


def check_sides(plan):
    """rows on either side of line 2^20: one line in forty matches, so the first batch has some 26000 rows; the second
    batch has 1500 lines, some 37 rows"""
    front = plan.rows_in_front_of(BATCH)
    assert front > 10000 and len(plan.lines) - front > 20, (front, len(plan.lines))
    return front


def cut_in_the_second_batch(plan):
    k = plan.rows_in_front_of(BATCH) + 7
    assert BATCH < int(plan.lines[k]) < NMANY
    return k


def test_two_default_batches_filter(gpu):
    buf = many_lines()
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, DIGIT)
        tables = filter_tables(exp, buf.pool, 0x0A, FIRST)
        assert int(tables[0].sum()) == len(K_LINES)
        sc = S.Scanner(pool, prog, FIRST)
        assert sc.engine == S.ENGINE_SCAN
        src = upload_at(buf.data, 3)
        try:
            base, n = src.ptr + 3, len(buf.data)
            for invert, all_lines in [(False, False), (True, False), (False, True)]:
                plan = Plan(buf, tables, invert, all_lines)
                if not invert and not all_lines:
                    check_sides(plan)
                else:
                    assert len(plan.lines) > NMANY - 30000
                call = filter_call(sc, base, n, invert=invert, all_lines=all_lines)
                bulk_run(gpu, plan, base, buf.data, call)                   # the whole index
                assert sc.last_line_batches == 2 and sc.last_lines_device == 1
                k = cut_in_the_second_batch(plan)
                info = bulk_run(gpu, plan, base, buf.data, call, out_cap=plan.ends[k] - 1, index_cap=9)
                assert info.nwritten == k and sc.last_line_batches == 2
        finally:
            src.free()


def test_two_default_batches_extract_and_substitute(gpu):
    buf = many_lines()
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, DIGIT)
        sc = S.Scanner(pool, prog, FIRST)
        assert sc.engine == S.ENGINE_SCAN and max_group(sc) == ncaps
        src = upload_at(buf.data, 3)
        try:
            base, n = src.ptr + 3, len(buf.data)
            tables = extract_tables(exp, buf.pool, 0x0A, [1, 0])
            assert per_lane(buf.n * 2) == 3
            plan = Plan(buf, tables)
            check_sides(plan)
            call = extract_call(sc, base, n, [1, 0])
            bulk_run(gpu, plan, base, buf.data, call)
            assert sc.last_line_batches == 2 and sc.last_lines_device == 1
            k = cut_in_the_second_batch(plan)
            info = bulk_run(gpu, plan, base, buf.data, call, out_cap=plan.ends[k - 1], index_cap=9)
            assert info.nwritten == k and sc.last_line_batches == 2

            tables = subst_tables(exp, buf.pool, 0x0A, b"<$1>", ncaps)
            assert per_lane(buf.n * 5) == 6                                 # "<", $1, ">" and the two ends of the line
            for all_lines in (False, True):
                plan = Plan(buf, tables, all_lines=all_lines)
                call = subst_call(sc, base, n, b"<$1>", all_lines=all_lines)
                bulk_run(gpu, plan, base, buf.data, call)
                assert sc.last_line_batches == 2 and sc.last_lines_device == 1
                k = cut_in_the_second_batch(plan)
                info = bulk_run(gpu, plan, base, buf.data, call, out_cap=plan.ends[k] - 1, index_cap=9)
                assert info.nwritten == k and sc.last_line_batches == 2
        finally:
            src.free()


def test_two_default_batches_scan_lines(gpu):
    buf = many_lines()
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, DIGIT)
        plan = Plan(buf, filter_tables(exp, buf.pool, 0x0A, FIRST))
        front = check_sides(plan)
        recs = [exp.record(line, FIRST) for line in buf.pool]
        want = [[i, st, ln] + recs[c] for i, st, ln, c in zip(plan.lines.tolist(), buf.start[plan.lines].tolist(),
                                                              buf.len[plan.lines].tolist(), buf.cid[plan.lines].tolist())]
        sc = S.Scanner(pool, prog, FIRST)
        assert sc.engine == S.ENGINE_SCAN
        src = upload_at(buf.data, 3)
        try:
            base, n = src.ptr + 3, len(buf.data)
            nl, nr, rows = sc.scan_lines(base, n, cap=NMANY + 1)
            assert sc.last_line_batches == 2 and sc.last_lines_device == 1
            assert (nl, nr) == (NMANY, len(want))
            assert rows == want, [(g, w) for g, w in zip(rows, want) if g != w][:3]
            assert sc.scan_lines(base, n, all_lines=True, cap=0) == (NMANY, NMANY, [])
            assert sc.last_line_batches == 2 and sc.last_lines_device == 1
            cap = front + 7                                                 # the cap ends inside the second batch
            assert want[cap - 1][0] > BATCH and cap < len(want)
            assert sc.scan_lines(base, n, cap=cap) == (NMANY, len(want), want[:cap])
            assert sc.last_line_batches == 2 and sc.last_lines_device == 1
        finally:
            src.free()


def test_two_batches_on_the_nfa_tier(gpu):
    """the short-line kernel with i0 > 0: every line is short.  For first match the batch may be smaller than 2^20
    lines (SRE_LINES_NFA_WORK_MAX / the stride of the window contexts), so there may be more than two"""
    buf = many_lines()
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, DOTTED)
        src = upload_at(buf.data, 3)
        try:
            base, n = src.ptr + 3, len(buf.data)
            sc = S.Scanner(pool, prog, S.HIP_THOMPSON, S.ENGINE_NFA)
            assert sc.engine == S.ENGINE_NFA
            tables = filter_tables(exp, buf.pool, 0x0A, S.HIP_THOMPSON)
            assert int(tables[0].sum()) == len(DOTTED_LINES)
            plan = Plan(buf, tables)
            check_sides(plan)
            bulk_run(gpu, plan, base, buf.data, filter_call(sc, base, n))
            print("thompson: batches", sc.last_line_batches)
            assert sc.last_short_lines == NMANY and sc.last_line_batches >= 2 and sc.last_lines_device == 1

            sc = S.Scanner(pool, prog, FIRST, S.ENGINE_NFA)
            assert sc.engine == S.ENGINE_NFA and max_group(sc) == ncaps
            plan = Plan(buf, extract_tables(exp, buf.pool, 0x0A, [1, 0]))
            bulk_run(gpu, plan, base, buf.data, extract_call(sc, base, n, [1, 0]))
            print("first match: batches", sc.last_line_batches)
            assert sc.last_short_lines == NMANY and sc.last_line_batches >= 2 and sc.last_lines_device == 1
            plan = Plan(buf, subst_tables(exp, buf.pool, 0x0A, b"[$1$0]", ncaps), all_lines=True)
            call = subst_call(sc, base, n, b"[$1$0]", all_lines=True)
            k = cut_in_the_second_batch(plan)
            info = bulk_run(gpu, plan, base, buf.data, call, out_cap=plan.ends[k - 1], index_cap=NMANY)
            assert info.nwritten == k
            assert sc.last_short_lines == NMANY and sc.last_line_batches >= 2 and sc.last_lines_device == 1
        finally:
            src.free()


# ------------------------------------------------------------------ 3. batches cut by the device

SEG = 1 << 18
CUT = WALK_MAX // (2 * (SEG + 16))      # sre_k_lines_plan: the most lines whose scratch fits
NCUT = 7000
G3 = [2, 0, 4]
T3 = b"<$2|$1>"


def uri_pool():
    rng = random.Random(18)
    pool = [b""]
    while len(pool) < 300:
        n = rng.randrange(1, 301)
        line = b" ".join(rng.choice(WORDS) for _ in range(n // 4 + 1))[:n]
        if line not in pool:
            pool.append(line)
    return pool


@functools.lru_cache(maxsize=None)
def cut_lines():
    """7000 lines of 0 .. 300 bytes: batches of 2047, 2047, 2047 and 859 lines under a segment of 2^18 bytes"""
    assert CUT == 2047 and CUT * (SEG + 16) * 2 <= WALK_MAX < (CUT + 1) * (SEG + 16) * 2
    assert [min(CUT, NCUT - i) for i in range(0, NCUT, CUT)] == [2047, 2047, 2047, 859]
    rng = random.Random(19)
    pool = uri_pool()
    cid = [rng.randrange(len(pool)) for _ in range(NCUT)]
    cid[-1] = 1
    buf = Lines(pool, cid)
    assert int(buf.len.max()) == 300 and int(buf.len.min()) == 0
    return buf


NBATCHES = -(-NCUT // CUT)


class CutScanner:
    """one scanner under the fixed segment (the device cuts the batches), then under the default one (one batch)"""

    def __init__(self, pool, prog):
        self.sc = S.Scanner(pool, prog, FIRST)
        assert self.sc.engine == S.ENGINE_SCAN

    def each(self, nbatches=NBATCHES):
        """sets the segment size; yields the batches a call then has to take"""
        for seg, want in ((SEG, nbatches), (0, 1)):
            self.sc.set_segment_bytes(seg)
            yield want

    def reached(self, want):
        """Another count than ceil(lines / 2047) means that sre_k_lines_plan no longer admits (i1 - i0) lines by
        (i1 - i0) * (seg + 16) * 2 <= SRE_LINES_WALK_MAX under a fixed segment: a finding, not a bound to relax"""
        assert self.sc.last_line_batches == want and self.sc.last_lines_device == 1, self.sc.last_line_batches
        return True


def test_cut_batches_scan_lines(gpu):
    buf = cut_lines()
    assert NBATCHES == 4
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, URI)
        cs = CutScanner(pool, prog)
        src = upload_at(buf.data, 3)
        try:
            base, n = src.ptr + 3, len(buf.data)
            for all_lines in (True, False):
                seen = []
                for want in cs.each():
                    rows = check(cs.sc, exp, buf.data, 0x0A, FIRST, all_lines, offset=3, batched=False)
                    cs.reached(want)
                    nr = len(rows)
                    assert all_lines or CUT + 1 < nr < NCUT
                    for cap in (1, CUT - 1, CUT, CUT + 1, nr - 1):
                        assert cs.sc.scan_lines(base, n, all_lines=all_lines, cap=cap) == (NCUT, nr, rows[:cap])
                        cs.reached(want)
                    seen.append(rows)
                assert seen[0] == seen[1]
        finally:
            src.free()


def test_cut_batches_filter(gpu):
    buf = cut_lines()
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, URI)
        cs = CutScanner(pool, prog)
        for invert, all_lines in [(False, False), (True, False), (False, True)]:
            seen = []
            for want in cs.each():
                seen.append(run_filter(cs.sc, exp, buf.data, 0x0A, FIRST, 3, 5, invert=invert, all_lines=all_lines))
                cs.reached(want)
            assert seen[0] == seen[1] and 0 < seen[0][0].nselected <= NCUT
        cs.sc.set_segment_bytes(SEG)
        sizes = [ln + 1 for _, _, ln in filter_expected(exp, buf.data, 0x0A, FIRST, all_lines=True)]
        for k in (CUT - 1, CUT, CUT + 1):
            info, _ = run_filter(cs.sc, exp, buf.data, 0x0A, FIRST, 3, 5, all_lines=True, out_cap=sum(sizes[:k]))
            assert info.nwritten == k and cs.reached(NBATCHES)
        for all_lines in (False, True):
            info, _ = run_filter(cs.sc, exp, buf.data, 0x0A, FIRST, 3, 5, all_lines=all_lines, index_cap=CUT)
            assert info.nwritten > CUT and cs.reached(NBATCHES)


def test_cut_batches_extract(gpu):
    buf = cut_lines()
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, URI)
        cs = CutScanner(pool, prog)
        for all_lines in (False, True):
            seen = []
            for want in cs.each():
                seen.append(run_extract(cs.sc, exp, buf.data, G3, src_off=3, dst_off=5, all_lines=all_lines)[:2])
                cs.reached(want)
            assert seen[0] == seen[1] and 0 < seen[0][0].nselected <= NCUT
        cs.sc.set_segment_bytes(SEG)
        sizes = [len(row_text(buf.data, f, 0x09, 0x0A)) for _, _, _, f in extract_expected(exp, buf.data, 0x0A, G3, True)]
        for k in (CUT - 1, CUT, CUT + 1):
            info, _, _ = run_extract(cs.sc, exp, buf.data, G3, src_off=3, dst_off=5, all_lines=True, out_cap=sum(sizes[:k]))
            assert info.nwritten == k and cs.reached(NBATCHES)
        for all_lines in (False, True):
            info, _, _ = run_extract(cs.sc, exp, buf.data, G3, src_off=3, dst_off=5, all_lines=all_lines, index_cap=CUT)
            assert info.nwritten > CUT and cs.reached(NBATCHES)


def test_cut_batches_substitute(gpu):
    buf = cut_lines()
    with S.Pool() as pool:
        prog, ncaps, exp = program(pool, URI)
        cs = CutScanner(pool, prog)
        assert max_group(cs.sc) == ncaps
        for all_lines in (False, True):
            seen = []
            for want in cs.each():
                seen.append(run_subst(cs.sc, exp, buf.data, T3, src_off=3, dst_off=5, all_lines=all_lines)[:2])
                cs.reached(want)
            assert seen[0] == seen[1] and 0 < seen[0][0].nselected <= NCUT
        cs.sc.set_segment_bytes(SEG)
        sizes = [len(row) + 1 for _, _, _, _, row in subst_expected(exp, buf.data, 0x0A, pieces_of(T3, ncaps), True)]
        for k in (CUT - 1, CUT, CUT + 1):
            info, _, _ = run_subst(cs.sc, exp, buf.data, T3, src_off=3, dst_off=5, all_lines=True, out_cap=sum(sizes[:k]))
            assert info.nwritten == k and cs.reached(NBATCHES)
        for all_lines in (False, True):
            info, _, _ = run_subst(cs.sc, exp, buf.data, T3, src_off=3, dst_off=5, all_lines=all_lines, index_cap=CUT)
            assert info.nwritten > CUT and cs.reached(NBATCHES)


LONG = 300000


@pytest.mark.parametrize("front", [CUT - 1, CUT], ids=["last-of-its-batch", "first-of-its-batch"])
def test_a_long_line_at_a_cut(gpu, front):
    """a line of two segments as the last line of the first batch, and as the first line of the second one; its match
    is at its far end, so the substitute copies the 300000 bytes in front of it"""
    rng = random.Random(21)
    pool = uri_pool()
    tail = b" zz://host/path?q=1"         # (the blank: the letters of the filler would be part of the scheme)
    long_line = bytes(rng.choice(b"xyw ") for _ in range(LONG - len(tail))) + tail
    assert SEG < len(long_line) == LONG <= 2 * SEG
    lines = [rng.choice(pool) for _ in range(front)] + [long_line] + [rng.choice(pool[1:]) for _ in range(60)]
    data = b"\n".join(lines)
    assert split_lines(data, 0x0A)[front][1] == LONG
    assert (front // CUT, front % CUT) == ((0, CUT - 1) if front == CUT - 1 else (1, 0))
    nbatches = -(-len(lines) // CUT)
    assert nbatches == 2
    with S.Pool() as pool_:
        prog, ncaps, exp = program(pool_, URI)
        cs = CutScanner(pool_, prog)
        m = [m for i, _, _, m, _ in subst_expected(exp, data, 0x0A, pieces_of(T3, ncaps), False) if i == front]
        assert m and m[0][0] - split_lines(data, 0x0A)[front][0] == LONG - len(tail) + 1
        for want in cs.each(nbatches):
            for all_lines in (False, True):
                check(cs.sc, exp, data, 0x0A, FIRST, all_lines, offset=3, batched=False)
                cs.reached(want)
                run_subst(cs.sc, exp, data, T3, src_off=3, dst_off=5, all_lines=all_lines)
                cs.reached(want)
            run_filter(cs.sc, exp, data, 0x0A, FIRST, 3, 5)
            cs.reached(want)
            run_extract(cs.sc, exp, data, G3, src_off=3, dst_off=5)
            cs.reached(want)


# ------------------------------------------------------------------ 4. the bulk path against the helpers

def test_the_bulk_path_agrees_with_the_helpers(gpu):
    """the same calls over the first 1500 lines of each large buffer through run_filter / run_extract / run_subst and
    through bulk_run: both compare the whole output and the whole index with their expectation, so the two
    expectations are the same"""
    with S.Pool() as pool:
        for buf, pats, groups, template in [(table_lines(NTABLE).head(1500), DIGIT, K32, T30),
                                            (many_lines().head(1500), DIGIT, [1, 0], b"<$1>")]:
            prog, ncaps, exp = program(pool, pats)
            sc = S.Scanner(pool, prog, FIRST)
            src = upload_at(buf.data, 3)
            try:
                base, n = src.ptr + 3, len(buf.data)
                tables = filter_tables(exp, buf.pool, 0x0A, FIRST)
                for invert, all_lines in [(False, False), (True, False), (False, True)]:
                    plan = Plan(buf, tables, invert, all_lines)
                    cap = plan.need // 2
                    for out_cap in (None, cap):
                        a = bulk_run(gpu, plan, base, buf.data, filter_call(sc, base, n, invert=invert, all_lines=all_lines),
                                     out_cap=out_cap)
                        b, _ = run_filter(sc, exp, buf.data, 0x0A, FIRST, 3, 5, invert, all_lines, out_cap=out_cap)
                        assert a == b
                for all_lines in (False, True):
                    plan = Plan(buf, extract_tables(exp, buf.pool, 0x0A, groups), all_lines=all_lines)
                    for out_cap in (None, plan.need // 2):
                        a = bulk_run(gpu, plan, base, buf.data, extract_call(sc, base, n, groups, all_lines=all_lines),
                                     out_cap=out_cap)
                        b, _, _ = run_extract(sc, exp, buf.data, groups, src_off=3, dst_off=5, all_lines=all_lines, out_cap=out_cap)
                        assert a == b
                    plan = Plan(buf, subst_tables(exp, buf.pool, 0x0A, template, ncaps), all_lines=all_lines)
                    for out_cap in (None, plan.need // 2):
                        a = bulk_run(gpu, plan, base, buf.data, subst_call(sc, base, n, template, all_lines=all_lines),
                                     out_cap=out_cap)
                        b, _, _ = run_subst(sc, exp, buf.data, template, src_off=3, dst_off=5, all_lines=all_lines, out_cap=out_cap)
                        assert a == b
            finally:
                src.free()
