"""Stream sets (sre_hip_streams_*): many device-resident streams of one program, fed chunk by
chunk, all together in one call.

Expected values come from the oracle fed the same calls (harness.OracleEngine), or from entry
points this feature does not touch (Scanner.scan, the compat API) — never from the stream set.
"""
import ctypes
import json
import os
import random
import time

import pytest

import sregex_amd as S
import harness

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("SRE_FUZZ_SEED", "0"))
SIZES = [0, 1, 7, 64, 255, 256, 1000, 4096, 10000, 33333]
CFG3 = [b"a", b"ab", b"c", b"a(bc)", b"e(f)", b"gh", b"A", b"b", b"BLAH", rb"\s+", b"abcd", b"bc"]
# the zoo, the tails and the alphabets of test_compat_api_chunked_streams_take_the_scanner
ZOO = [[rb"[a-z]+@[a-z]+\.[a-z]+"], [rb"([a-z]+)://([^/ ]+)(/[^ ?]*)?(\?[^ ]*)?"], [rb"a?a?a?aaa"],
       [rb"(a+)(b+)?"], [rb"(?:a.*b|a)"], [rb"x(.*)y(.*)z"], [rb"(a|ab)(c|bcd)(d*)"], CFG3,
       [rb"\Aab|\n^b"], [rb"(x+x+)+y"], [rb"^b+"], [rb"q(\w+)@"],
       [rb"\bab\b"], [rb"(a+)$"], [rb"(\w+)\b(.)"], [rb"c\B(.)"], [rb"^(\w+) \b"], [rb"x*\b y"]]
TAILS = [b"@abc.cc ", b" abc://abc.cc/ab/c?a=b ", b"aaabbccb", b" a\nca", b"xabyabz", b"q"]
ALPHABETS = [b"abc", b"ab c\n.x@:/?y", b"aaaaab xy\nz"]
NSTREAMS = 96


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def has_lookahead(pats):
    return any(tok in p for p in pats for tok in (b"$", b"\\b", b"\\B", b"\\z"))


def subjects(rng, n):
    """n subjects: gen-data streams with the six tails, random text over the three alphabets"""
    out = []
    for i in range(n):
        if i % 2 == 0:
            out.append(S.gen_data_host(rng.choice([900, 9000, 40000]), TAILS[(i // 2) % len(TAILS)]))
        else:
            alpha = ALPHABETS[(i // 2) % len(ALPHABETS)]
            out.append(bytes(rng.choice(alpha) for _ in range(rng.choice([300, 5000, 20000]))))
    return out


def schedule(rng, length):
    """chunk sizes of one stream: a few drawn sizes, then the rest with eof — [(offset, size, eof)]"""
    out, off = [], 0
    sizes = [rng.choice(SIZES) for _ in range(rng.randrange(0, 9))]
    while True:
        n = min(sizes.pop(0) if sizes else length - off, length - off)
        eof = off + n >= length and not sizes
        out.append((off, n, eof))
        off += n
        if eof:
            return out


class OracleStream:
    """one oracle context fed the calls of one stream; expect() is the record of a call"""

    def __init__(self, ora, prog, ncaps, thompson):
        self.thompson = thompson
        self.nov = 2 * (ncaps + 1)
        self.ctx = ora.thompson(prog) if thompson else ora.pike(prog, ncaps)
        self.closed = None          # the closing record's defined part

    def call(self, chunk, eof):
        """(rc, state, pending triple, {slot: value} of the defined ovector slots)"""
        if self.closed is not None:
            rc, _, pend, ov = self.closed
            return rc, S.StreamSet.WAS_CLOSED, pend, ov
        if self.thompson:
            rc = self.ctx.exec(chunk, eof)
            rec = (rc, 0 if rc == S.SRE_AGAIN else 1, (0, -1, -1), {})
        else:
            rc = self.ctx.exec(chunk, eof, want_pending=True)
            if rc == S.SRE_AGAIN:
                pend = (1,) + tuple(self.ctx.pending) if self.ctx.pending else (0, -1, -1)
                rec = (rc, 0, pend, {0: self.ctx.ovector[0], 1: self.ctx.ovector[1]})
            else:
                ov = {k: self.ctx.ovector[k] for k in range(self.nov)} if rc >= 0 else {}
                rec = (rc, 1, (0, -1, -1), ov)
        if rec[1] == 1:
            self.closed = rec
            self.ctx.close()
        return rec

    def close(self):
        if self.closed is None:
            self.ctx.close()


def check_record(rec, want, ctx):
    rc, state, pend, ov = want
    assert rec[0] == rc and rec[1] == state, (ctx, rec, want)
    assert tuple(rec[2:5]) == tuple(pend), (ctx, rec, want)
    for k, v in ov.items():
        assert rec[5 + k] == v, (ctx, k, rec, want)


def run_schedules(gpu, pool, prog, ncaps, mode, subs, scheds, rng, idle=0.2, engine=None):
    """feed every stream its schedule, all streams in each call; returns the number of
    (stream, call) pairs compared with the oracle.  engine: the engine the set must run on"""
    ora = harness.OracleEngine()
    n = len(subs)
    blob = b"#" + b"".join(subs)            # natural (odd) offsets
    offs, o = [], 1
    for s in subs:
        offs.append(o)
        o += len(s)
    buf = S.DeviceBuffer.from_bytes(blob)
    ss = S.StreamSet(pool, prog, mode, n)
    assert ss.n == n and ss.slots == 5 + 2 * (ncaps + 1)
    assert engine is None or ss.engine == engine, (ss.engine, engine)
    streams = [OracleStream(ora, prog, ncaps, mode == S.HIP_THOMPSON) for _ in range(n)]
    nxt = [0] * n
    compared = 0
    last = [None] * n
    while any(nxt[i] < len(scheds[i]) for i in range(n)):
        ptrs, lens, eofs, fed = [None] * n, [0] * n, [0] * n, [None] * n
        for i in range(n):
            if nxt[i] < len(scheds[i]) and rng.random() >= idle:
                off, k, eof = scheds[i][nxt[i]]
                nxt[i] += 1
                ptrs[i], lens[i], eofs[i] = buf.ptr + offs[i] + off, k, eof
                fed[i] = (off, k, eof)
        recs = ss.feed(ptrs, lens, eofs)
        for i in range(n):
            if fed[i] is None:
                assert recs[i][1] == S.StreamSet.NOT_FED, (i, recs[i])
                continue
            off, k, eof = fed[i]
            want = streams[i].call(subs[i][off:off + k], eof)
            check_record(recs[i], want, (i, len(subs[i]), fed[i], scheds[i][:nxt[i]], last[i]))
            last[i] = recs[i]
            compared += 1
    for s in streams:
        s.close()
    buf.free()
    return compared


@pytest.mark.parametrize("mode", [S.HIP_PIKE_FIRST, S.HIP_THOMPSON])
def test_every_call_equals_the_oracles_call(gpu, mode):
    """96 streams per program with different subjects and chunk schedules; one call mixes first,
    middle, EOF and empty chunks with idle and closed streams.  Every record of every fed stream
    equals what the oracle answered to the same call."""
    rng = random.Random(5151 + SEED + mode)
    programs = compared = generated = 0
    for pats in ZOO:
        if mode == S.HIP_THOMPSON and has_lookahead(pats):
            continue
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            subs = subjects(rng, NSTREAMS)
            scheds = [schedule(rng, len(s)) for s in subs]
            generated += sum(len(s) for s in scheds)
            compared += run_schedules(gpu, pool, prog, re.ncaps, mode, subs, scheds, rng)
            programs += 1
    assert programs == (len(ZOO) if mode == S.HIP_PIKE_FIRST else sum(not has_lookahead(p) for p in ZOO))
    assert compared == generated, (compared, generated)     # no case skipped


def test_fixup_rounds_inside_a_set(gpu, monkeypatch):
    """small segments, so that streams have many lanes whose speculative entry states can be
    wrong: the set runs its fix-up rounds and still answers as the oracle does"""
    monkeypatch.setenv("SRE_HIP_SEG_BYTES", "256")
    rng = random.Random(77 + SEED)
    seen = 0
    for pats in ([rb"x(.*)y(.*)z"], [rb"(a+)$"], [rb"x(?:[^y]{3})*y"]):
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            subs = [bytes(rng.choice(b"abxy \n") for _ in range(rng.choice([3000, 9000]))) for _ in range(24)]
            scheds = [schedule(rng, len(s)) for s in subs]
            assert run_schedules(gpu, pool, prog, re.ncaps, S.HIP_PIKE_FIRST, subs, scheds, rng) == sum(map(len, scheds))
            seen += 1
    assert seen == 3
    # subjects that are known to defeat speculation (test_scanner_fixup_rounds_are_reported,
    # test_scanner_automaton_that_never_forgets_gets_exact_entry_states), beside neighbours that
    # settle at once: the rounds must run (last_fixups >= 1) and every record equal the oracle's
    ora = harness.OracleEngine()
    cases = [([rb"(?:a.*b|a)"], b"xx a" + b"c" * 5000 + b"b" + b"c" * 3000, 4000),
             ([rb"x(?:[^y]{3})*y"], b"ab" * 50 + b"x" + b"abc" * 4000 + b"ab" + b"y" + b"zz", 7001)]
    for pats, hard, cut in cases:
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            subs = [b"c" * 6000, hard, b"q" * 9000, hard[50:], b""]
            cuts = [3000, cut, 1, cut - 50, 0]
            bufs = [S.DeviceBuffer.from_bytes(x) for x in subs]
            ss = S.StreamSet(pool, prog, S.HIP_PIKE_FIRST, len(subs))
            o = [OracleStream(ora, prog, re.ncaps, False) for _ in subs]
            fixups = 0
            for call in range(2):
                lo = [0 if call == 0 else c for c in cuts]
                hi = [c if call == 0 else len(x) for c, x in zip(cuts, subs)]
                recs = ss.feed([b.ptr + a for b, a in zip(bufs, lo)], [b - a for a, b in zip(lo, hi)], [call] * len(subs))
                fixups += ss.last_fixups
                for i, x in enumerate(subs):
                    check_record(recs[i], o[i].call(x[lo[i]:hi[i]], call == 1), (pats, call, i))
            assert fixups >= 1, (pats, fixups)
            for s_ in o:
                s_.close()
            for b in bufs:
                b.free()


def test_lookahead_across_chunk_boundaries(gpu):
    """every split position of a 64-byte window around the match, all in ONE call sequence as
    different streams, against the oracle fed the same way"""
    rng = random.Random(1)
    cases = [([rb"a(\s\B.)?"], b"." * 4094 + b"a b"),
             ([rb"\bab\b"], b"#" * 200 + b"xab ab ab_ " + b"#" * 50),
             ([rb"(a+)$"], b"b" * 150 + b"aaa\nbaa" + b"b" * 20 + b"aa"),
             ([rb"^(\w+) \b"], b"# " * 80 + b"\nfoo_1 bar\nbaz #" + b" " * 40)]
    ora = harness.OracleEngine()
    for pats, data in cases:
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            whole = ora.pike(prog, re.ncaps)
            rc = whole.exec(data, True)
            assert rc >= 0, (pats, rc)
            end = whole.ovector[1]
            lo, hi = max(0, end - 48), min(len(data), end + 16)
            if pats == [rb"a(\s\B.)?"]:
                # whole (4094, 4095); split behind the blank (4094, 4097)
                assert tuple(whole.ovector[:2]) == (4094, 4095)
                w2 = harness.OracleEngine().pike(prog, re.ncaps)
                assert w2.exec(data[:4096], False) == S.SRE_AGAIN and w2.exec(data[4096:], True) == 0
                assert tuple(w2.ovector[:2]) == (4094, 4097)
                lo, hi = 4064, len(data)
            splits = list(range(lo, hi + 1))
            subs = [data] * len(splits)
            scheds = [[(0, p, False), (p, len(data) - p, True)] for p in splits]
            n = run_schedules(gpu, pool, prog, re.ncaps, S.HIP_PIKE_FIRST, subs, scheds, rng, idle=0.0)
            assert n == 2 * len(splits)


def test_admission(gpu):
    with S.Pool() as pool:
        def prog_of(pats):
            return S.compile(pool, S.parse(pool, pats))
        with pytest.raises(RuntimeError):
            S.StreamSet(pool, prog_of([rb"$\A\nb"]), S.HIP_THOMPSON, 4)
        nfa = prog_of([rb"(?:a|b)*a(?:a|b){7}@"])
        assert S.Scanner(pool, nfa, S.HIP_PIKE_FIRST, S.ENGINE_AUTO).engine == S.ENGINE_NFA
        for mode in (S.HIP_PIKE_FIRST, S.HIP_THOMPSON):
            with pytest.raises(RuntimeError):
                S.StreamSet(pool, nfa, mode, 4)
        with pytest.raises(RuntimeError):
            S.StreamSet(pool, prog_of([rb"(a+)$"]), S.HIP_PIKE_COUNT, 4)
        ss = S.StreamSet(pool, prog_of([rb"(a+)$"]), S.HIP_PIKE_FIRST, 4)
        assert ss.n == 4 and ss.slots == 5 + 4 and ss.device_bytes > 0


def test_reset_gives_a_slot_a_fresh_context(gpu):
    ora = harness.OracleEngine()
    pats = [rb"([a-z]+)@([a-z]+)\.[a-z]+"]
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        a = S.gen_data_host(6000, b" x@abc.cc ")
        b = b"#" * 700 + b" bob@example.com " + b"#" * 100
        c = S.gen_data_host(9000, b"aaabbccb")
        bufs = [S.DeviceBuffer.from_bytes(x) for x in (a, b, c)]
        ss = S.StreamSet(pool, prog, S.HIP_PIKE_FIRST, 3)
        o = [OracleStream(ora, prog, re.ncaps, False) for _ in range(3)]
        # streams 0 and 2 mid-search, stream 1 closed by a match
        recs = ss.feed([bufs[0].ptr, bufs[1].ptr, bufs[2].ptr], [3001, len(b), 4000], [0, 1, 0])
        check_record(recs[0], o[0].call(a[:3001], False), 0)
        check_record(recs[1], o[1].call(b, True), 1)
        check_record(recs[2], o[2].call(c[:4000], False), 2)
        assert recs[1][0] == 0 and recs[1][1] == S.StreamSet.CLOSED
        recs = ss.feed([None, bufs[1].ptr, None], [0, 5, 0], [0, 0, 0])
        assert recs[1][1] == S.StreamSet.WAS_CLOSED and recs[1][0] == 0
        ss.reset([1])
        o[1] = OracleStream(ora, prog, re.ncaps, False)        # a new flow takes over the slot
        recs = ss.feed([bufs[0].ptr + 3001, bufs[2].ptr + 100, bufs[2].ptr + 4000], [len(a) - 3001, 3000, len(c) - 4000],
                       [1, 0, 1])
        check_record(recs[0], o[0].call(a[3001:], True), 0)
        check_record(recs[1], o[1].call(c[100:3100], False), 1)
        check_record(recs[2], o[2].call(c[4000:], True), 2)
        assert recs[0][0] == 0 and recs[2][0] == S.SRE_DECLINED and recs[1][0] == S.SRE_AGAIN
        for x in bufs:
            x.free()


def test_one_call_many_shapes(gpu):
    """4096 streams of 0-300 bytes, fed whole with eof in one call: rc and ovector of the batched
    API (unchanged code) on the same pointers"""
    rng = random.Random(99 + SEED)
    n = 4096
    for pats in ([rb"([a-z]+)@([a-z]+)\.[a-z]+"], [rb"(a+)$"], CFG3):
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            lens = [rng.randrange(0, 301) for _ in range(n)]
            blob = bytes(rng.choice(b"ab c\n.x@e") for _ in range(sum(lens) + 1))
            buf = S.DeviceBuffer.from_bytes(blob)
            ptrs, o = [], 1
            for k in lens:
                ptrs.append(buf.ptr + o)
                o += k
            want = S.Scanner(pool, prog, S.HIP_PIKE_FIRST).scan(ptrs, lens)
            got = S.StreamSet(pool, prog, S.HIP_PIKE_FIRST, n).feed(ptrs, lens, [1] * n)
            for i in range(n):
                assert got[i][0] == want[i][0] and got[i][1] == S.StreamSet.CLOSED, (i, got[i], want[i])
                assert got[i][2:5] == [0, -1, -1], (i, got[i])
                assert got[i][5:] == want[i][2:], (i, got[i], want[i])
            buf.free()


@pytest.mark.parametrize("tail", [b"@abc.cc ", b" a@abc.cc "])
def test_offsets_beyond_4_gib(gpu, tail):
    """One stream of the headline program fed a little over 4 GiB from ONE reused device buffer of
    64 MiB - 4 bytes (a multiple of 5: the abccc period continues from call to call), the last
    chunk ending in the tail.  The expected records are the closed form the oracle gives for a
    20 000-byte stream under the same kind of chunking, scaled.  A second stream of 1 KiB, fed in
    the first call only, is not disturbed by its long neighbour."""
    ora = harness.OracleEngine()
    pats = [rb"[a-z]+@[a-z]+\.[a-z]+"]
    carried = tail == b"@abc.cc "       # the match starts at offset 0 of the stream, else in the last chunk
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        # the closed form, from the oracle on a small stream chunked the same way
        small_chunk, small_n = 2000, 10
        body = b"abccc" * (small_chunk // 5)
        lastc = S.gen_data_host(small_chunk, tail)
        o = ora.pike(prog, re.ncaps)
        for k in range(small_n - 1):
            assert o.exec(body, False) == S.SRE_AGAIN
            assert tuple(o.ovector[:2]) == (0, -1) and o.pending is None, (k, list(o.ovector), o.pending)
        assert o.exec(lastc, True) == 0
        small_total = (small_n - 1) * small_chunk + len(lastc)
        start_of = lambda total: 0 if carried else total - 9
        assert tuple(o.ovector[:2]) == (start_of(small_total), small_total - 1), (list(o.ovector), small_total)

        chunk = (64 << 20) - 4
        assert chunk % 5 == 0
        ncalls = (1 << 32) // chunk + 2            # a little over 4 GiB
        buf = S.DeviceBuffer(chunk)
        assert gpu.sre_hip_gen_data(buf.ptr, chunk, b"", 0, None) == 0
        assert gpu.sre_hip_synchronize(None) == 0
        short = S.gen_data_host(1024, b" x@abc.cc ")
        sbuf = S.DeviceBuffer.from_bytes(short)
        so = ora.pike(prog, re.ncaps)
        assert so.exec(short, True) == 0
        ss = S.StreamSet(pool, prog, S.HIP_PIKE_FIRST, 2)
        for k in range(ncalls - 1):
            recs = ss.feed([buf.ptr, sbuf.ptr if k == 0 else None], [chunk, len(short) if k == 0 else 0], [0, 1])
            assert recs[0][:7] == [S.SRE_AGAIN, 0, 0, -1, -1, 0, -1], (k, recs[0])
            if k == 0:
                assert recs[1] == [0, 1, 0, -1, -1] + list(so.ovector[:2]), recs[1]
            else:
                assert recs[1][1] == S.StreamSet.NOT_FED
        last_len = S.gen_data_length(chunk, len(tail))
        assert gpu.sre_hip_gen_data(buf.ptr, last_len, tail, len(tail), None) == 0
        assert gpu.sre_hip_synchronize(None) == 0
        recs = ss.feed([buf.ptr, sbuf.ptr], [last_len, 3], [1, 0])
        total = (ncalls - 1) * chunk + last_len
        assert total > 1 << 32
        assert recs[0] == [0, 1, 0, -1, -1, start_of(total), total - 1], (recs[0], total)
        assert recs[0][6] > 1 << 32 and (carried or recs[0][5] > 1 << 32)
        assert recs[1] == [0, S.StreamSet.WAS_CLOSED, 0, -1, -1] + list(so.ovector[:2]), recs[1]
        buf.free()
        sbuf.free()


def test_the_host_does_not_work_per_stream(gpu):
    """the launches and copies of a call are the same for 8 and for 8192 fed streams"""
    pats = [rb"[a-z]+@[a-z]+\.[a-z]+"]
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        data = S.gen_data_host(16384, b" a@abc.cc ")
        buf = S.DeviceBuffer.from_bytes(data)
        counts = {}
        for n in (8, 8192):
            want = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
            want.scan([buf.ptr] * n, [len(data)] * n)
            assert want.last_fixups == 0
            ss = S.StreamSet(pool, prog, S.HIP_PIKE_FIRST, n)
            recs = ss.feed([buf.ptr] * n, [8000] * n, [0] * n)
            assert all(r[0] == S.SRE_AGAIN for r in recs)
            assert ss.last_fixups == 0
            first = ss.last_launches
            recs = ss.feed([buf.ptr + 8000] * n, [len(data) - 8000] * n, [1] * n)
            assert all(r[:2] == [0, 1] and r[5:7] == [len(data) - 9, len(data) - 1] for r in recs), recs[0]
            assert ss.last_fixups == 0
            counts[n] = (first, ss.last_launches)
        assert counts[8] == counts[8192] and counts[8][0] > 0, counts
        buf.free()


def test_rate_sanity_against_the_compat_api(gpu):
    """1024 streams x 1 MiB chunks x 8 calls through the set move more bytes per second than the
    compat API feeds ONE stream in 1 MiB chunks from host memory (the measurement of
    test_compat_api_chunked_stream_rate).  The margin is 1x on purpose: it catches a set that
    serialises its streams."""
    pats, tail = [rb"[a-z]+@[a-z]+\.[a-z]+"], b" a@abc.cc "
    chunk, nstreams, ncalls = 1 << 20, 1024, 8
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        # the compat API: one stream of 64 MiB in 1 MiB chunks from host memory, second pass timed
        data = S.gen_data_host(64 << 20, tail)
        L = len(data)
        hbuf = ctypes.create_string_buffer(data, L)
        compat = None
        for _ in range(2):
            with S.Pool() as ep:
                ctx = S.PikeCtx(ep, prog, re.ncaps)
                t0 = time.perf_counter()
                off, rc = 0, S.SRE_AGAIN
                while rc == S.SRE_AGAIN:
                    k = min(chunk, L - off)
                    rc = ctx.exec(None, off + k >= L, want_pending=False, base=hbuf, offset=off, length=k)
                    off += k
                compat = L / (time.perf_counter() - t0) / 1e9
                assert rc == 0 and list(ctx.ovector) == [L - 9, L - 1]
        # the set: the streams' chunks are slices of one 1 GiB device buffer without a match
        big = S.DeviceBuffer(nstreams * chunk)
        assert gpu.sre_hip_gen_data(big.ptr, nstreams * chunk, b"", 0, None) == 0
        assert gpu.sre_hip_synchronize(None) == 0
        ss = S.StreamSet(pool, prog, S.HIP_PIKE_FIRST, nstreams)
        ptrs = (ctypes.c_void_p * nstreams)(*[big.ptr + i * chunk for i in range(nstreams)])
        lens = (ctypes.c_size_t * nstreams)(*([chunk] * nstreams))
        eofs = (ctypes.c_ubyte * nstreams)(*([0] * nstreams))
        ss.feed_raw(ptrs, lens, eofs)       # warm-up: the set's per-call buffers
        t0 = time.perf_counter()
        for _ in range(ncalls):
            out = ss.feed_raw(ptrs, lens, eofs)
        rate = ncalls * nstreams * chunk / (time.perf_counter() - t0) / 1e9
        assert all(out[i * ss.slots] == S.SRE_AGAIN for i in range(nstreams))
        big.free()
    row = {"set_GBps": rate, "compat_one_stream_GBps": compat, "ratio": rate / compat,
           "streams": nstreams, "chunk": chunk, "calls": ncalls}
    # (printed; profiles/streams_rate.json keeps the row of the run it records as rate_sanity_test)
    print("stream set vs compat API:", json.dumps(row))
    assert rate > compat, row
