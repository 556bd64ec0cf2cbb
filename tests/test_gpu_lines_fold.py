"""The line fold (sre_hip_fold_lines): continuation lines joined into multi-line records, from one device buffer to another.

Expected output is pure Python: the split rule of line mode, the oracle's verdict on every line, and the header's
definitions (a line is MARKED when it has a match, with invert when it has none; a natural head is line 0 or, by default, a
line that is not marked, with fold_next a line whose predecessor is not marked; max_lines splits a record into pieces).
Every output and table buffer has the filter tests' guard bytes and 0xA5 fill; every check asserts the guards and
everything at or beyond what the call may write.
"""
import ctypes
import random

import pytest

import sregex_amd as S
from hipstream import GatedStream
from test_gpu_caller_stream import Src, call_filter, gated_check, kv_pair, kvw_scanner, line_cap, run as run_outs
from test_gpu_lines import Expect, split_lines, upload_at
from test_gpu_lines_context import edge_buffer, headline
from test_gpu_lines_filter import LENGTHS, ROUTES, Out, download, random_lines, small_buffer
from test_gpu_nfa_wide import WIDE

pytestmark = pytest.mark.gpu

N_EDGE = 3 * 1024 + 17
MODES = [(nxt, inv) for nxt in (False, True) for inv in (False, True)]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def fold(marked, nxt, max_lines):
    """head(i) of every line, from the definitions"""
    heads, h = [], 0
    for i in range(len(marked)):
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
    sets = [[False] * 60, [True] * 60, [k in (0, 7, 8, 30, 59) for k in range(60)]] + [[rng.random() < p for _ in range(60)]
                                                                                      for p in (0.1, 0.5, 0.9)]
    for m in sets:
        for nxt in (False, True):
            for cap in (0, 1, 2, 3, 7, 59, 60, 61, (1 << 64) - 1):
                assert fold(m, nxt, cap) == by_definition(m, nxt, cap)


def words(lib, ptr, nwords):
    return list((ctypes.c_int64 * nwords).from_buffer_copy(download(lib, ptr, 8 * nwords))) if nwords else []


class Case:
    """one source buffer on the device with the oracle's verdict on each of its lines (computed once)"""

    def __init__(self, sc, exp, data, mode, delim=0x0A, src_off=0, hits=None):
        self.sc, self.lib, self.data, self.delim, self.src_off = sc, sc.lib, data, delim, src_off
        self.lines = split_lines(data, delim)
        self.hits = hits if hits is not None else [exp.record(data[st:st + n], mode)[0] != S.SRE_DECLINED for st, n in self.lines]
        self.src = upload_at(data, src_off)
        self.ptr = self.src.ptr + src_off

    def free(self):
        self.src.free()

    def expected(self, join, max_lines, invert, nxt):
        """(heads, records [(first line, lines, source offset, bytes without the final delimiter, output offset)], text)"""
        marked = [h != invert for h in self.hits]
        heads = fold(marked, nxt, max_lines)
        n = len(self.lines)
        firsts = [i for i in range(n) if heads[i]]
        recs, o = [], 0
        for a, b in zip(firsts, firsts[1:] + [n]):
            size = sum(k + 1 for _, k in self.lines[a:b])
            recs.append((a, b - a, self.lines[a][0], size - 1, o))
            o += size
        d, j = bytes([self.delim]), bytes([join])
        text = b"".join(self.data[st:st + k] + (d if i == n - 1 or heads[i + 1] else j) for i, (st, k) in enumerate(self.lines))
        return marked, heads, recs, text

    def run(self, join=0x01, max_lines=0, invert=False, nxt=False, dst_off=0, out_cap=None, recid_cap=None, records_cap=None,
            null_out=False, hip_stream=None):
        """one call, checked in full; returns (info, output bytes, records rows)"""
        n = len(self.lines)
        marked, heads, recs, text = self.expected(join, max_lines, invert, nxt)
        need = len(text)
        assert need == sum(k for _, k in self.lines) + n
        cap = need + 37 if out_cap is None else out_cap
        nwritten = 0
        while nwritten < len(recs) and recs[nwritten][4] + recs[nwritten][3] + 1 <= cap:
            nwritten += 1
        out_bytes = recs[nwritten][4] if nwritten < len(recs) else need
        want = text[:out_bytes]
        icap = n + 3 if recid_cap is None else recid_cap
        rcap = len(recs) + 3 if records_cap is None else records_cap
        out = Out(self.lib, cap, dst_off)
        rid = Out(self.lib, 8 * icap, 0)
        rec = Out(self.lib, 40 * rcap, 0)
        try:
            info = self.sc.fold_lines(self.ptr, len(self.data), None if null_out else out.ptr, cap, join, max_lines, self.delim, invert,
                                      nxt, rid.ptr if icap else None, icap, rec.ptr if rcap else None, rcap, hip_stream)
            longest = max(r[1] for r in recs) if recs else 0
            assert info == S.FoldInfo(n, sum(marked), len(recs), longest, need, nwritten, out_bytes), (info, len(recs), nwritten, cap)
            out.check(want)
            nid = min(icap, n)
            ids, r = [], -1
            for i in range(nid):
                r += heads[i]
                ids.append(r)
            assert words(self.lib, rid.ptr, nid) == ids
            rid.check(download(self.lib, rid.ptr, 8 * nid))         # nothing behind the words, nothing around the table
            nrows = min(rcap, nwritten)
            raw = words(self.lib, rec.ptr, 5 * nrows)
            got = [tuple(raw[5 * k:5 * k + 5]) for k in range(nrows)]
            assert got == recs[:nrows], [(g, w) for g, w in zip(got, recs) if g != w][:3]
            rec.check(download(self.lib, rec.ptr, 40 * nrows))
        finally:
            out.free()
            rid.free()
            rec.free()
        return info, want, recs[:nrows]


# ------------------------------------------------------------------ 1. edges of the buffer, the waves and the workgroups

SPOTS = [0, 255, 256, 1023, 1024, 2047, 2048, N_EDGE - 1]


@pytest.mark.parametrize("nxt,inv", MODES, ids=["prev", "prev-invert", "next", "next-invert"])
def test_edges(gpu, nxt, inv):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        assert sc.engine == S.ENGINE_SCAN
        cases = [Case(sc, exp, edge_buffer(SPOTS, final), S.HIP_PIKE_FIRST) for final in (False, True)]
        try:
            assert all(len(c.lines) == N_EDGE and sum(c.hits) == len(SPOTS) for c in cases)
            for k, max_lines in enumerate([0, 1, 3, 1024, 1025]):
                for c in cases:
                    info, _, recs = c.run(max_lines=max_lines, invert=inv, nxt=nxt, dst_off=k)
                    if inv and not nxt and max_lines == 0:
                        assert [r[0] for r in recs] == SPOTS and info.longest == N_EDGE - 1 - 2048       # the planted heads
                    if max_lines:
                        assert info.longest <= max_lines
            assert sc.last_lines_device == 1
        finally:
            for c in cases:
                c.free()


# ------------------------------------------------------------------ 2. alignment, lengths, join and delimiter bytes

def lengths_buffer(rng, delim, final_delim):
    """lines of LENGTHS (and their neighbours) without the delimiter; every second one holds a K"""
    alphabet = bytes(b for b in b"xyw q" if b != delim)
    lines = []
    for i, n in enumerate(LENGTHS + [3, 0, 0, 70]):
        line = bytearray(rng.choice(alphabet) for _ in range(n))
        if i % 2 and n:
            line[rng.randrange(n)] = ord("K")
        lines.append(bytes(line))
    d = bytes([delim])
    return d.join(lines) + (d if final_delim else b"")


def test_alignment_lengths_join_and_delimiter(gpu):
    rng = random.Random(77)
    with S.Pool() as pool:
        re = S.parse(pool, [rb"K"])
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps)
        sc = S.Scanner(pool, prog, S.HIP_THOMPSON)
        for delim in (0x0A, 0x7C):
            data = lengths_buffer(rng, delim, delim == 0x0A)
            hits = None
            for src_off in (0, 1, 15, 16):
                c = Case(sc, exp, data, S.HIP_THOMPSON, delim=delim, src_off=src_off, hits=hits)
                hits = c.hits
                try:
                    assert 0 < sum(hits) < len(c.lines) == len(LENGTHS) + 4
                    for k, dst_off in enumerate((0, 1, 15, 16)):
                        join = (0x01, 0x20, 0x00, delim)[(k + src_off) % 4]
                        nxt, inv = MODES[k]
                        info, want, _ = c.run(join=join, invert=inv, nxt=nxt, dst_off=dst_off)
                        if join == delim:       # the input with a final delimiter
                            assert want == data + (b"" if data.endswith(bytes([delim])) else bytes([delim]))
                        c.run(join=join, max_lines=2, invert=inv, nxt=nxt, dst_off=dst_off)
                finally:
                    c.free()


# ------------------------------------------------------------------ 3. truncation and the tables' capacities

def test_truncation(gpu):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        c = Case(sc, exp, small_buffer(9), S.HIP_PIKE_FIRST, src_off=1)
        try:
            assert len(c.lines) == 120
            for nxt, inv in [(False, True), (True, False)]:
                _, _, recs, text = c.expected(0x01, 0, inv, nxt)
                need = len(text)
                assert 10 < len(recs) < 120 and max(r[1] for r in recs) > 2
                caps = {need + 37, need, 0, 1}
                for r in recs:
                    end = r[4] + r[3] + 1
                    caps |= {end - 1, end, end + 1}
                for cap in sorted(caps, reverse=True):
                    info, _, _ = c.run(invert=inv, nxt=nxt, dst_off=cap % 16, out_cap=cap)
                    assert info.need_bytes == need and info.out_bytes <= cap and info.nrecords == len(recs)
                # the sizing call: no output buffer at all
                info, _, _ = c.run(invert=inv, nxt=nxt, out_cap=0, null_out=True)
                assert (info.nwritten, info.out_bytes, info.need_bytes) == (0, 0, need)
                # tables at 0, at 1, short and exact, each alone and together
                for icap, rcap in [(0, 0), (1, 1), (0, len(recs)), (120, 0), (57, 7), (120, len(recs)), (119, len(recs) - 1)]:
                    info, _, rows = c.run(invert=inv, nxt=nxt, recid_cap=icap, records_cap=rcap)
                    assert len(rows) == rcap
                info, _, rows = c.run(invert=inv, nxt=nxt, out_cap=need // 2, records_cap=3)
                assert 3 < info.nwritten < len(recs) and len(rows) == 3
        finally:
            c.free()


# ------------------------------------------------------------------ 4. every route

@pytest.mark.parametrize("name,pats,mode,engine,routed,device", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route(gpu, name, pats, mode, engine, routed, device):
    data = random_lines(5)
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        exp = Expect(prog, re.ncaps, key=("filter", tuple(pats)))
        sc = S.Scanner(pool, prog, mode, engine)
        assert sc.engine == routed
        if name.startswith("nfa-wide"):
            assert sc.nfa_bits == WIDE[1][1]
        c = Case(sc, exp, data, mode, src_off=3)
        try:
            assert 0 < sum(c.hits) < len(c.lines) == 2000
            for nxt, inv in [(False, False), (True, True)]:
                info, _, _ = c.run(invert=inv, nxt=nxt, dst_off=5)
                assert sc.last_lines_device == device and sc.last_line_batches >= 1
                assert 1 < info.nrecords < info.nlines and info.longest > 1
            c.run(max_lines=2, invert=True, dst_off=5)
        finally:
            c.free()


# ------------------------------------------------------------------ 5. several batches

def test_several_batches(gpu, monkeypatch):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        c = Case(sc, exp, small_buffer(12, nlines=100), S.HIP_PIKE_FIRST, src_off=2)
        try:
            assert len(c.lines) == 100
            one = [c.run(invert=inv, nxt=nxt, dst_off=9) for nxt, inv in MODES]
            assert sc.last_line_batches == 1
            monkeypatch.setenv("SRE_HIP_LINES_BATCH", "7")
            for (nxt, inv), (info1, want1, recs1) in zip(MODES, one):
                # a record straddles a batch cut
                assert any(a < cut < a + k for a, k, _, _, _ in recs1 for cut in range(7, 100, 7))
                assert c.run(invert=inv, nxt=nxt, dst_off=9) == (info1, want1, recs1)
                assert sc.last_line_batches == 15
        finally:
            c.free()


# ------------------------------------------------------------------ 6. composition with the other sinks

def synthetic_log(seed, nrecords=500):
    """records of a timestamped head and 0 .. 6 indented frame lines; some carry a cause; every line names its request"""
    rng = random.Random(seed)
    records = []
    for k in range(nrecords):
        req = b"req-%d" % rng.randrange(8)
        lines = [b"2024-03-%02d 12:%02d:%02d ERROR [%s] request failed" % (1 + k % 28, k % 60, rng.randrange(60), req)]
        for f in range(rng.randrange(0, 7)):
            lines.append(b"\tat com.foo.Bar.method%d(Bar.java:%d) [%s]" % (f, rng.randrange(999), req))
        if rng.random() < 0.3:
            lines.insert(rng.randrange(1, len(lines) + 1), b"Caused by: java.io.IOException: broken pipe [%s]" % req)
        records.append(lines)
    return records


def test_composition_with_filter_and_tally(gpu):
    records = synthetic_log(4)
    data = b"".join(b"\n".join(r) + b"\n" for r in records)
    folded = b"".join(b"\x01".join(r) + b"\n" for r in records)
    nlines = sum(len(r) for r in records)
    with S.Pool() as pool:
        stamp = S.Scanner(pool, S.compile(pool, S.parse(pool, [rb"^\d{4}-\d\d-\d\d"])), S.HIP_THOMPSON)
        cont = S.Scanner(pool, S.compile(pool, S.parse(pool, [rb"^(\s|Caused by:)"])), S.HIP_THOMPSON)
        ioex = S.Scanner(pool, S.compile(pool, S.parse(pool, [rb"IOException"])), S.HIP_PIKE_FIRST)
        reqs = S.Scanner(pool, S.compile(pool, S.parse(pool, [rb"\[(req-\d)\]"])), S.HIP_PIKE_FIRST)
        src = S.DeviceBuffer.from_bytes(data)
        mid, out, cnt = S.DeviceBuffer(len(data) + 16), S.DeviceBuffer(len(data) + 16), S.DeviceBuffer(8 * 16)
        try:
            # both spellings of "what is not a head belongs to the previous line"
            for sc, invert in ((stamp, True), (cont, False)):
                info = sc.fold_lines(src.ptr, len(data), mid.ptr, mid.nbytes, join=0x01, invert=invert)
                assert info == S.FoldInfo(nlines, nlines - 500, 500, max(len(r) for r in records), len(data), 500, len(data))
                assert mid.to_bytes(info.out_bytes) == folded
            # grep on the folded buffer selects whole records, with their frames
            f = ioex.filter_lines(mid.ptr, len(folded), out.ptr, out.nbytes)
            want = [b"\x01".join(r) + b"\n" for r in records if any(b"IOException" in x for x in r)]
            assert 100 < f.nselected == len(want) < 250 and out.to_bytes(f.out_bytes) == b"".join(want)
            assert all(x.startswith(b"2024-") and b"Caused by" in x for x in want)
            # on the source it finds orphan lines
            f0 = ioex.filter_lines(src.ptr, len(data), out.ptr, out.nbytes)
            assert f0.nselected == len(want) and all(x.startswith(b"Caused by") for x in out.to_bytes(f0.out_bytes).split(b"\n")[:-1])
            # a tally on the request of the head line counts records on the folded buffer, lines on the source
            t = reqs.tally_lines(mid.ptr, len(folded), out.ptr, out.nbytes, [1], 16, counts_ptr=cnt.ptr, counts_cap=16)
            keys = out.to_bytes(t.out_bytes).split(b"\n")[:-1]
            counts = dict(zip(keys, (ctypes.c_uint64 * t.nkeys).from_buffer_copy(cnt.to_bytes(8 * t.nkeys))))
            per_req = {}
            for r in records:
                k = r[0][r[0].index(b"[") + 1:r[0].index(b"]")]
                per_req[k] = per_req.get(k, 0) + 1
            assert counts == per_req and sum(counts.values()) == 500 == t.nselected
            t0 = reqs.tally_lines(src.ptr, len(data), out.ptr, out.nbytes, [1], 16)
            assert t0.nselected == nlines > 500
        finally:
            for b in (src, mid, out, cnt):
                b.free()


# ------------------------------------------------------------------ 7. idempotence and neighbours

def test_folding_the_output_again_reproduces_it_and_the_neighbours_stand(gpu):
    with S.Pool() as pool:
        sc, exp = headline(pool)
        data = small_buffer(10, nlines=400, final_delim=True)
        c = Case(sc, exp, data, S.HIP_PIKE_FIRST)
        out = S.DeviceBuffer(len(data) + 64)
        idx = S.DeviceBuffer(40 * 401)
        try:
            def neighbours():
                f = sc.filter_lines(c.ptr, len(data), out.ptr, out.nbytes, index_ptr=idx.ptr, index_cap=401)
                a = (f, out.to_bytes(f.out_bytes), idx.to_bytes(32 * f.nwritten))
                g = sc.filter_lines_context(c.ptr, len(data), out.ptr, out.nbytes, 1, 2, index_ptr=idx.ptr, index_cap=401)
                b = (g, out.to_bytes(g.out_bytes), idx.to_bytes(40 * g.nwritten))
                return a, b, sc.scan_lines(c.ptr, len(data), cap=401)

            before = neighbours()
            # the program matches anywhere in a line, so a folded line has a match when any of its source lines had one
            for nxt, inv in MODES:
                info, once, _ = c.run(join=0x01, invert=inv, nxt=nxt)
                c2 = Case(sc, exp, once, S.HIP_PIKE_FIRST, src_off=3)
                try:
                    info2, twice, _ = c2.run(join=0x01, invert=inv, nxt=nxt)
                    assert info2.nlines == info.nrecords
                    if (nxt, inv) == (False, True):
                        # heads are the lines with a match: a record starts with one (but for line 0, which may have
                        # none), so every folded line is a head again
                        assert twice == once and info2.nrecords == info.nrecords and info2.nmarked <= 1
                finally:
                    c2.free()
            assert neighbours() == before
        finally:
            c.free()
            out.free()
            idx.free()


def test_idempotence_on_a_log(gpu):
    """the head rule reads the start of a line only, so the folded buffer folds to itself under every mapping of it"""
    records = synthetic_log(8, 300)
    data = b"".join(b"\n".join(r) + b"\n" for r in records)
    with S.Pool() as pool:
        re = S.parse(pool, [rb"^\d{4}-\d\d-\d\d"])
        prog = S.compile(pool, re)
        sc, exp = S.Scanner(pool, prog, S.HIP_PIKE_FIRST), Expect(prog, re.ncaps)
        c = Case(sc, exp, data, S.HIP_PIKE_FIRST)
        try:
            info, once, _ = c.run(join=0x01, invert=True)
            assert info.nrecords == 300 and once == b"".join(b"\x01".join(r) + b"\n" for r in records)
            c2 = Case(sc, exp, once, S.HIP_PIKE_FIRST, src_off=5)
            try:
                info2, twice, _ = c2.run(join=0x01, invert=True, dst_off=3)
                assert twice == once and (info2.nlines, info2.nrecords, info2.nmarked, info2.longest) == (300, 300, 0, 1)
            finally:
                c2.free()
        finally:
            c.free()


# ------------------------------------------------------------------ 8. the caller's stream

def call_fold(sc, src, n, hs, spans):
    L = line_cap(n)
    return run_outs(sc, [n + L + 16, 8 * L, 40 * L], lambda out, rid, rec: sc.fold_lines(
        src, n, out.ptr, out.cap, recid_ptr=rid.ptr, recid_cap=L, records_ptr=rec.ptr, records_cap=L, hip_stream=hs))


def test_on_a_gated_stream_with_its_producer_pending(gpu):
    real, decoy = (Src(t) for t in kv_pair(21))
    try:
        with S.Pool() as pool:
            got, sc = gated_check(lambda: kvw_scanner(pool), call_fold, real, decoy)
            assert sc.engine == S.ENGINE_SCAN and sc.last_lines_device == 1
            assert 1 < got[0].nrecords < got[0].nlines
    finally:
        real.free()
        decoy.free()


@pytest.mark.parametrize("fold_first", [True, False], ids=["fold-filter", "filter-fold"])
def test_interleaved_with_filter_lines_on_a_callers_stream(gpu, fold_first):
    texts = [Src(t) for t in kv_pair(23)]
    s = GatedStream()
    try:
        with S.Pool() as pool:
            calls = [call_fold, call_filter] if fold_first else [call_filter, call_fold]
            fresh = {(k, j): calls[k](kvw_scanner(pool), t.ptr, len(t.data), None, t.lines) for k in (0, 1) for j, t in enumerate(texts)}
            sc = kvw_scanner(pool)
            for k, j in [(0, 0), (1, 1), (0, 0), (1, 0), (0, 1), (1, 1)]:
                t = texts[j]
                assert calls[k](sc, t.ptr, len(t.data), s.handle, t.lines) == fresh[k, j], (k, j)
    finally:
        s.close()
        for t in texts:
            t.free()
