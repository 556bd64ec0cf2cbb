"""Compact segment records of first-match and Thompson scans (sregex_amd/csrc/sre_scan_record.h): the scan kernel writes
a 16-byte digest for every segment and the 136-byte record only where the digest does not say it all; the grid-wide
chain check (sre_k_verify_a / b / b2) reads digests alone, every other reader rebuilds a plain segment's record from
its digest.  The summary buffer is reused from call to call, so behind a plain digest lies whatever an earlier call
wrote there.

Every expected record comes from the oracle (_expect of tests/test_gpu_parity.py); ENGINE_SCAN is forced.  The shapes are
the smallest that take the grid-wide check and not the one-workgroup one: small inputs get 256-byte segments and one
workgroup checks up to 8192 of them, so a single stream is 8200 to 8900 segments (a little over 2 MiB) and the batch is
three streams that pass 8192 together.  What an input is meant to hold (no match, where the match lies) is asserted on
the oracle's record before the GPU is asked.  tests/test_scan_record_model.py checks the pack / load rule itself on
the CPU."""
import pytest

import sregex_amd as S
import harness
from test_gpu_parity import _expect
from test_gpu_scan_forms import URI, compare, scanners, MODES

pytestmark = pytest.mark.gpu

SEG = 256                   # segment size of a small input
ONE = 8192                  # most segments the one-workgroup chain check takes
EMAIL = rb"([a-z]+)@([a-z]+)\.[a-z]+"
ROTATING = rb"x(?:[^y]{3})*y"
FIRST_MODES = (S.HIP_PIKE_FIRST, S.HIP_THOMPSON)


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def body(nseg, extra=0):
    """nseg whole segments (and `extra` bytes) of the benchmark's filler: no match of EMAIL or URI, one stable state"""
    return S.gen_data_host(nseg * SEG + extra, b"")


def put(data, at, ev):
    out = bytearray(data)
    out[at:at + len(ev)] = ev
    return bytes(out)


class Case:
    """one program, its scanners, the oracle"""

    def __init__(self, pool, pats, modes=MODES):
        self.pats = pats
        self.re = S.parse(pool, pats)
        self.prog = S.compile(pool, self.re)
        self.scs = scanners(pool, self.prog, modes)
        assert set(self.scs) == set(modes), (pats, sorted(self.scs))
        self.ora = harness.OracleEngine()

    def expect(self, data):
        return _expect(self.ora, self.prog, self.re.ncaps, data)

    def check(self, datas, expect, modes=None, ctx=None):
        """one call per mode over all of datas, every record against the oracle's; the segment size and the count of
        segments are the grid-wide check's"""
        bufs = [S.DeviceBuffer.from_bytes(d) for d in datas]
        try:
            for mode, sc in self.scs.items():
                if modes is not None and mode not in modes:
                    continue
                got = sc.scan([b.ptr for b in bufs], [len(d) for d in datas])
                assert sc.last_segment_bytes == SEG, sc.last_segment_bytes
                assert sum((len(d) + SEG - 1) // SEG for d in datas) > ONE
                for i, (first, cnt) in enumerate(expect):
                    compare(got, mode, i, first, cnt, (self.pats, ctx, i, len(datas[i])))
        finally:
            for b in bufs:
                b.free()


def test_no_match_every_record_but_the_last_is_plain(gpu):
    with S.Pool() as pool:
        c = Case(pool, [EMAIL])
        for data in (body(8200), body(8193, 77)):
            exp = c.expect(data)
            assert exp[0][0] == S.SRE_DECLINED and exp[1][1] == 0
            c.check([data], [exp])


@pytest.mark.parametrize("where", ["first", "middle", "last", "straddle"])
def test_match_position(gpu, where):
    """a whole match inside the first, a middle and the last segment, and one that straddles a segment boundary: the
    records around it are plain, its own is not"""
    nseg = 8300
    at = {"first": 40, "middle": 4111 * SEG + 100, "last": (nseg - 1) * SEG + 90, "straddle": 5000 * SEG - 4}[where]
    data = put(body(nseg), at, b" x@abc.cc ")
    with S.Pool() as pool:
        c = Case(pool, [EMAIL])
        exp = c.expect(data)
        # " x@abc.cc " at `at`: the match is [at + 1, at + 9)
        assert exp[0][:4] == [0, 1, at + 1, at + 9], exp[0]
        assert ((at + 1) // SEG != (at + 8) // SEG) == (where == "straddle")
        assert (at + 1) // SEG == {"first": 0, "middle": 4111, "last": nseg - 1, "straddle": 4999}[where]
        c.check([data], [exp], ctx=where)


@pytest.mark.parametrize("pat", [EMAIL, URI], ids=["email", "uri"])
def test_match_spanning_the_stream(gpu, pat):
    """the match ends at the end of the stream and begins at its start: the capture walker crosses thousands of plain
    segments by their rebuilt stable_until"""
    tail = b"@abc.cc " if pat == EMAIL else b"://abc.cc/ab/c?a=b "
    if pat == EMAIL:
        data = S.gen_data_host(8400 * SEG + 8, tail)
    else:
        data = b"a" * (8400 * SEG) + tail
    with S.Pool() as pool:
        c = Case(pool, [pat])
        exp = c.expect(data)
        assert exp[0][0] == 0 and exp[0][2] == 0 and exp[0][3] >= len(data) - 2, exp[0]
        c.check([data], [exp])


def test_stale_buffer(gpu):
    """One scanner: a call whose every segment carries an event (a match every 200 bytes, so the stream ends early), a
    call in which no match completes but most segments are not stable ('@' without its tail in every segment), then a
    call of the same geometry with no match at all.  Its records equal a fresh scanner's and the oracle's: nothing
    of the earlier calls' records is read behind the plain digests."""
    nseg = 8500
    dense = (b"a@b.c" + b" " * 195) * (nseg * SEG // 200 + 1)
    dense = dense[:nseg * SEG]
    unstable = bytearray(body(nseg))
    for k in range(nseg):
        if k % 7 != 3:
            unstable[k * SEG + 100] = ord("@")
    unstable = bytes(unstable)
    quiet = body(nseg)
    with S.Pool() as pool:
        c = Case(pool, [EMAIL], FIRST_MODES)
        e_dense, e_unst, e_quiet = c.expect(dense), c.expect(unstable), c.expect(quiet)
        assert e_dense[0][0] == 0 and e_dense[0][3] == 5 and e_dense[1][1] > nseg
        assert e_unst[0][0] == S.SRE_DECLINED and e_quiet[0][0] == S.SRE_DECLINED
        bufs = [S.DeviceBuffer.from_bytes(d) for d in (dense, unstable, quiet)]
        try:
            for mode, sc in c.scs.items():
                for buf, data, exp in zip(bufs, (dense, unstable, quiet), (e_dense, e_unst, e_quiet)):
                    got = sc.scan([buf.ptr], [len(data)])
                    assert sc.last_segment_bytes == SEG
                    compare(got, mode, 0, exp[0], exp[1], (mode, len(data)))
                    last = got
                fresh = S.Scanner(pool, c.prog, mode, S.ENGINE_SCAN).scan([bufs[2].ptr], [len(quiet)])
                assert last == fresh, (mode, last, fresh)
        finally:
            for b in bufs:
                b.free()


def test_program_that_breaks_speculation(gpu):
    """x(?:[^y]{3})*y behind an x: the state rotates with the input, every guess of an entry state is wrong two times
    in three, fix-up rounds and the composed entry states rewrite records that were plain and make plain ones of
    records that were not"""
    nseg = 8400
    cases = [b"ab" * 50 + b"x" + b"abc" * (nseg * SEG // 3) + b"ab" + b"y" + b"zz",
             b"ab" * 50 + b"x" + b"abc" * (nseg * SEG // 3) + b"abc" + b"y" + b"zz",
             b"abc" * (nseg * SEG // 3) + b"x" + b"abc" * 4000 + b"y"]
    with S.Pool() as pool:
        c = Case(pool, [ROTATING], FIRST_MODES)
        exps = [c.expect(d) for d in cases]
        assert exps[0][0][0] == S.SRE_DECLINED and exps[1][0][0] == 0 and exps[2][0][0] == 0, [e[0] for e in exps]
        for data, exp in zip(cases, exps):
            c.check([data], [exp], ctx=len(data))
        sc = c.scs[S.HIP_PIKE_FIRST]
        buf = S.DeviceBuffer.from_bytes(cases[0])
        try:
            sc.scan([buf.ptr], [len(cases[0])])
            assert sc.last_exact_passes >= 1, sc.last_exact_passes
        finally:
            buf.free()


def test_three_stream_batch(gpu):
    """three streams that pass 8192 segments together, matching and non-matching mixed; the first boundary between two
    streams lies inside one 1024-segment span of sre_k_verify_b (segment 3000 + 1 is no multiple of 1024)"""
    a = put(body(3000, 10), 2000 * SEG + 17, b" x@abc.cc ")
    b = body(3001, 100)
    c3 = S.gen_data_host(2400 * SEG + 8, b"@abc.cc ")
    datas = [a, b, c3]
    nsegs = [(len(d) + SEG - 1) // SEG for d in datas]
    assert sum(nsegs) > ONE and nsegs[0] % 1024 != 0 and (nsegs[0] + nsegs[1]) % 1024 != 0
    with S.Pool() as pool:
        c = Case(pool, [EMAIL])
        exps = [c.expect(d) for d in datas]
        assert [e[0][0] for e in exps] == [0, S.SRE_DECLINED, 0]
        c.check(datas, exps)
        # ... and in another order: the non-matching stream first
        c.check([b, c3, a], [exps[1], exps[2], exps[0]])


def test_count_mode_is_untouched(gpu):
    """one COUNT call on the inputs above: its kernels write and read whole records as before"""
    datas = [body(8200), put(body(8300), 4111 * SEG + 100, b" x@abc.cc "), S.gen_data_host(8400 * SEG + 8, b"@abc.cc ")]
    with S.Pool() as pool:
        c = Case(pool, [EMAIL], (S.HIP_PIKE_COUNT,))
        for d in datas:
            c.check([d], [c.expect(d)])
