"""Every device call on a caller's non-blocking stream (include/sregex_hip.h: "all its work runs on hip_stream").

CALLS is the table of every call kind the header declares, each in one uniform shape: call(sc, src_ptr, nbytes,
hip_stream, spans) allocates its own outputs (Out: guard bytes, 0xA5 throughout), makes the call with every optional
side array present, waits for nothing itself and returns (info, the bytes of every output with its guards, diagnostics);
spans are the lines of the text the call is to see, which only `scan` reads (its streams are host-side pointers).
A scanner of the table (kvw_scanner) carries what its calls need besides: .keys, the key set and key map of the keyed
calls, and .probe, which run() asks straight before it enters the library.  The downloads are synchronous copies on the null stream, which do not wait for a non-blocking stream: a call that
returned before its work was complete shows up as 0xA5 or stale bytes.

A gated case (hipstream.GatedStream) uploads a DECOY of the real input's length, queues on the caller's stream a closed
gate and behind it the copy of the real input over the decoy, and makes the call at once.  Work that the library issued
on another stream would run while the gate is closed and read the decoy, or scratch that has not been filled; a case
asserts that the null-stream answers on the real input and on the decoy differ, that the copy was still pending right
before the call, and that the whole reference call takes less than a tenth of the time the gate stays closed.  Expected
values are the same call on a fresh scanner on the null stream; the suites of each call kind tie those to the oracle.

What the gate decides and what it does not: a line call waits for the caller's stream when it reads the line count of
its split, so the gate is certain to be closed only for what the call issues up to that first wait; work issued on
another stream later in the call is no longer held back by the gate, only unordered against the caller's stream.
"""
import random
import threading
import time

import pytest

import sregex_amd as S
from hipstream import FIND_ALL_HOLD, HOLD, TABLE_SET_HOLD, GatedStream, timed
from test_gpu_lines import split_lines
from test_gpu_lines_filter import COUNTED, FILL, GUARD, Out
from test_gpu_lines_tally_sums import KVW, OCTETS, base6
from test_gpu_lines_tally_top import dotted_lines, top_lines
from test_gpu_streams import schedule

pytestmark = pytest.mark.gpu

SHORT_MAX = 512         # sre_hip_lines.h SRE_LINES_SHORT_MAX
# route_lines' program: four rules, no groups (a program of KVW and two more rules is too large for the table-driven scanner)
ROUTE4 = [rb"k=[a-c]", rb"k=[x-z][a-z]*;v=-", rb"k=[x-z]", rb"no key"]
ROUTE4_BUCKETS = [2, 0, 1, 0, 3]        # the lines without a match: bucket 3
ONE_RULE_BUCKETS = [2, 3]               # on a scanner of one rule (the call-order test): its lines and the others


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


# ------------------------------------------------------------------ inputs

class Src:
    """a text on the device and its lines"""

    def __init__(self, data):
        self.data = data
        self.lines = split_lines(data, 0x0A)
        self.buf = S.DeviceBuffer.from_bytes(data)

    @property
    def ptr(self):
        return self.buf.ptr

    def free(self):
        self.buf.free()


def padded(texts):
    """the texts with final lines of at most 60 bytes that hold no match, all of one length"""
    texts = [t.rstrip(b"\n") for t in texts]
    total = max(len(t) for t in texts) + 9
    out = []
    for t in texts:
        while len(t) < total:
            t += b"\n" + b"#" * min(total - len(t) - 1, 60)
        out.append(t)
    return out


def with_long_line(text, line):
    lines = text.rstrip(b"\n").split(b"\n")
    lines.insert(137, line)
    return b"\n".join(lines)


def kv_text(seed, extra):
    """about 300 lines k=KEY;v=NUMBER;w=TEXT; of under 100 bytes over 50 keys, a tenth of them without a match, v over
    a range that takes two digit passes, and one line longer than the short-line limit"""
    return with_long_line(top_lines(seed, 50, extra=extra, span=300), b"k=long;v=%d;w=" % seed + b"x" * 600 + b";")


def checked_pair(real, decoy, nlines=(250, 350)):
    real, decoy = padded([real, decoy])
    assert len(real) == len(decoy)
    for t in (real, decoy):
        lines = split_lines(t, 0x0A)
        assert nlines[0] <= len(lines) <= nlines[1] and sum(n > SHORT_MAX for _, n in lines) == 1
        assert len(lines) <= line_cap(len(t))
    assert len(split_lines(real, 0x0A)) != len(split_lines(decoy, 0x0A))
    return real, decoy


def kv_pair(seed):
    return checked_pair(kv_text(seed, 4.4), kv_text(seed + 100, 4.0))


def dotted_pair(seed):
    long_line = b"x " * 300 + b"9.9.9.9 ok"
    return checked_pair(with_long_line(dotted_lines(seed, 300), long_line), with_long_line(dotted_lines(seed + 100, 280), long_line))


def counted_text(seed, nlines):
    """lines of a, b and @ of up to 200 bytes for COUNTED, and one of 3000 bytes"""
    rng = random.Random(seed)
    lines = [bytes(rng.choice(b"aaabbb@") for _ in range(rng.randrange(0, 200))) for _ in range(nlines)]
    return with_long_line(b"\n".join(lines), bytes(rng.choice(b"aaabbb@") for _ in range(3000)))


def counted_pair(seed):
    return checked_pair(counted_text(seed, 300), counted_text(seed + 100, 280))


def line_cap(nbytes):
    """rows for every line of a text of the generators here (no line of theirs but the last is shorter than 8 bytes
    with its delimiter on average); checked_pair asserts it"""
    return nbytes // 4 + 8


# ------------------------------------------------------------------ the key set and the key map of the keyed calls

class Keys:
    """what a scanner of the table carries as .keys: the keyed calls read their key set and key map from it"""

    def __init__(self, set=None, map=None, rows=()):
        self.set, self.map, self.rows = set, map, rows


def dictionary_rows():
    """every second key of the generators, the long line's key and one key no text holds"""
    return [base6(j + 1) for j in range(0, 1025, 2)] + [b"long", b"zzzzzzz"]


def set_text(rows):
    return b"".join(k + b"\n" for k in rows)


def map_text(rows):
    return b"".join(k + b"\t" + b"V%d" % i + b"\t" + k.upper()[:3 + i % 5] + b"\n" for i, k in enumerate(rows))


@pytest.fixture(scope="module")
def keys(gpu):
    """the key set and the key map of the keyed calls, built on the null stream before any call that uses them"""
    rows = dictionary_rows()
    bufs = [S.DeviceBuffer.from_bytes(set_text(rows)), S.DeviceBuffer.from_bytes(map_text(rows))]
    made = []
    try:
        made.append(S.KeySet(bufs[0].ptr, bufs[0].nbytes, 1, lib=gpu))
        made.append(S.KeySet(bufs[1].ptr, bufs[1].nbytes, 3, lib=gpu, nkeys=1))
        assert made[0].distinct == made[1].distinct == len(rows) and made[1].values == 2
    finally:
        for b in bufs:
            b.free()
    yield Keys(made[0], made[1], rows)
    for ks in made:
        ks.close()


# ------------------------------------------------------------------ the call table

def run(sc, caps, fn, lines=True):
    """the Outs of `caps` bytes, info = fn(*outs), the bytes of every Out with its guards, the diagnostics.
    A scanner of the table carries .probe: asked straight before the library is entered, its answer kept as .probed (a
    gated case asks there whether its gate is closed); and .returned: when the library's call returned"""
    outs = []
    try:
        for cap in caps:
            outs.append(Out(sc.lib, cap, 0))
        sc.probed = sc.probe() if sc.probe else None
        info = fn(*outs)
        sc.returned = time.perf_counter()
        diag = (sc.last_line_batches, sc.last_lines_device, sc.last_short_lines) if lines else (sc.last_fixups,)
        return info, tuple(o.buf.to_bytes(o.total) for o in outs), diag
    finally:
        for o in outs:
            o.free()


def guards_intact(answer):
    fill = bytes([FILL]) * GUARD
    return all(raw[:GUARD] == fill and raw[-GUARD:] == fill for raw in answer[1] if isinstance(raw, bytes))


def kvw_scanner(pool, engine=S.ENGINE_AUTO, mode=S.HIP_PIKE_FIRST, pats=KVW, keys=None):
    """a scanner of the table: .keys is the Keys its keyed calls use; .probe, .probed and .returned are run()'s"""
    sc = S.Scanner(pool, S.compile(pool, S.parse(pool, pats)), mode, engine)
    sc.keys, sc.probe, sc.probed, sc.returned = keys, None, None, None
    return sc


def route_scanner(pool, keys=None):
    return kvw_scanner(pool, pats=ROUTE4, keys=keys)


def call_scan(sc, src, n, hs, spans):
    def fn():
        recs = sc.scan([src + st for st, _ in spans], [k for _, k in spans], hs)
        return (len(recs), sum(r[0] != S.SRE_DECLINED for r in recs)), tuple(map(tuple, recs))
    (info, recs), _, diag = run(sc, [], fn, lines=False)
    return info, (recs,), diag


def call_scan_lines(sc, src, n, hs, spans):
    def fn():
        nl, nr, rows = sc.scan_lines(src, n, all_lines=True, cap=line_cap(n), hip_stream=hs)
        return (nl, nr), tuple(map(tuple, rows))
    (info, rows), _, diag = run(sc, [], fn)
    return info, (rows,), diag


def call_filter(sc, src, n, hs, spans):
    L = line_cap(n)
    return run(sc, [n + 16, 32 * L], lambda out, idx: sc.filter_lines(src, n, out.ptr, out.cap, index_ptr=idx.ptr, index_cap=L,
                                                                       hip_stream=hs))


def call_context(sc, src, n, hs, spans):
    L = line_cap(n)
    return run(sc, [n + 16, 40 * L], lambda out, idx: sc.filter_lines_context(src, n, out.ptr, out.cap, before=1, after=2,
                                                                               index_ptr=idx.ptr, index_cap=L, hip_stream=hs))


def extract_call(groups):
    def call(sc, src, n, hs, spans):
        L = line_cap(n)
        return run(sc, [2 * n + 4 * L, 8 * (4 + 2 * len(groups)) * L],
                   lambda out, idx: sc.extract_lines(src, n, groups, out.ptr, out.cap, index_ptr=idx.ptr, index_cap=L, hip_stream=hs))
    return call


def call_substitute(sc, src, n, hs, spans):
    L = line_cap(n)
    return run(sc, [2 * n + 8 * L, 64 * L], lambda out, idx: sc.substitute_lines(src, n, b"<$1:$2>", out.ptr, out.cap, index_ptr=idx.ptr,
                                                                                 index_cap=L, hip_stream=hs))


def call_route(sc, src, n, hs, spans):
    L = line_cap(n)

    def fn(out, idx):
        info, buckets = sc.route_lines(src, n, out.ptr, out.cap, ROUTE4_BUCKETS if sc.nregexes == 4 else ONE_RULE_BUCKETS, 4, index_ptr=idx.ptr, index_cap=L, hip_stream=hs)
        return info, tuple(buckets)
    return run(sc, [n + 16, 40 * L], fn)


def tally_call(groups):
    K = len(groups)

    def call(sc, src, n, hs, spans):
        L = line_cap(n)
        return run(sc, [n + 16, 8 * L, 8 * L, 8 * (4 + 2 * K) * L],
                   lambda out, cnt, kid, idx: sc.tally_lines(src, n, out.ptr, out.cap, groups, L, counts_ptr=cnt.ptr, counts_cap=L,
                                                             keyid_ptr=kid.ptr, keyid_cap=L, index_ptr=idx.ptr, index_cap=L,
                                                             hip_stream=hs))
    return call


def sums_call(groups, vgroups):
    K, V = len(groups), len(vgroups)

    def call(sc, src, n, hs, spans):
        L = line_cap(n)
        return run(sc, [n + 16, 8 * L, 32 * V * L, 8 * L, 8 * (4 + 2 * K) * L],
                   lambda out, cnt, sums, kid, idx: sc.tally_sums_lines(src, n, out.ptr, out.cap, groups, vgroups, L, counts_ptr=cnt.ptr,
                                                                        counts_cap=L, sums_ptr=sums.ptr, sums_cap=L, keyid_ptr=kid.ptr,
                                                                        keyid_cap=L, index_ptr=idx.ptr, index_cap=L, hip_stream=hs))
    return call


def call_lookup(sc, src, n, hs, spans):
    L = line_cap(n)
    return run(sc, [n + 16, 8 * L, 32 * L],
               lambda out, kid, idx: sc.lookup_lines(src, n, out.ptr, out.cap, [1], sc.keys.set, keyid_ptr=kid.ptr, keyid_cap=L,
                                                     index_ptr=idx.ptr, index_cap=L, hip_stream=hs))


def call_join(sc, src, n, hs, spans):
    L = line_cap(n)
    return run(sc, [n + 24 * L, 8 * L, 8 * 9 * L],
               lambda out, kid, idx: sc.join_lines(src, n, out.ptr, out.cap, [1], sc.keys.map, [1, 0], all_lines=True, keyid_ptr=kid.ptr,
                                                   keyid_cap=L, index_ptr=idx.ptr, index_cap=L, hip_stream=hs))


def call_route_key(sc, src, n, hs, spans):
    L = line_cap(n)
    B = len(sc.keys.rows) + 2
    return run(sc, [n + 16, 8 * L, 40 * L, 40 * B],
               lambda out, kid, idx, bkt: sc.route_lines_by_key(src, n, out.ptr, out.cap, [1], sc.keys.set, all_lines=True, keyid_ptr=kid.ptr,
                                                                keyid_cap=L, index_ptr=idx.ptr, index_cap=L, buckets_ptr=bkt.ptr,
                                                                buckets_cap=B, hip_stream=hs))


def call_sort(sc, src, n, hs, spans):
    L = line_cap(n)
    return run(sc, [n + 16, 48 * L], lambda out, idx: sc.sort_lines(src, n, out.ptr, out.cap, 2, descending=True, all_lines=True,
                                                                    index_ptr=idx.ptr, index_cap=L, hip_stream=hs))


def top_call(groups, vgroups):
    K, V = len(groups), len(vgroups)

    def call(sc, src, n, hs, spans):
        L = line_cap(n)
        return run(sc, [n + 16, 8 * L, 32 * V * L, 8 * L, 8 * (6 + 2 * K) * L],
                   lambda out, cnt, sums, rnk, idx: sc.tally_top_lines(src, n, out.ptr, out.cap, groups, vgroups, L, S.HIP_TOP_SUM, 0, True,
                                                                       counts_ptr=cnt.ptr, counts_cap=L, sums_ptr=sums.ptr, sums_cap=L,
                                                                       rank_ptr=rnk.ptr, rank_cap=L, index_ptr=idx.ptr, index_cap=L,
                                                                       hip_stream=hs))
    return call


# (name, make_scanner(pool, keys), call(sc, src_ptr, nbytes, hip_stream, spans)); spans: the text's lines, which only `scan` reads
CALLS = [
    ("scan", kvw_scanner, call_scan),
    ("scan_lines", kvw_scanner, call_scan_lines),
    ("filter_lines", kvw_scanner, call_filter),
    ("filter_lines_context", kvw_scanner, call_context),
    ("extract_lines", kvw_scanner, extract_call([1, 2, 0])),
    ("substitute_lines", kvw_scanner, call_substitute),
    ("route_lines", route_scanner, call_route),
    ("tally_lines", kvw_scanner, tally_call([1])),
    ("tally_sums_lines", kvw_scanner, sums_call([1], [2, 3])),
    ("lookup_lines", kvw_scanner, call_lookup),
    ("join_lines", kvw_scanner, call_join),
    ("route_lines_by_key", kvw_scanner, call_route_key),
    ("sort_lines", kvw_scanner, call_sort),
    ("tally_top_lines", kvw_scanner, top_call([1], [2, 3])),
]
CALL_IDS = [c[0] for c in CALLS]


# ------------------------------------------------------------------ the gated check

def differ(want, want_decoy):
    """a stale read of the decoy cannot pass for the real input: the info and the output bytes both differ"""
    return want[0] != want_decoy[0] and want[1] != want_decoy[1]


def gated_check(make, call, real, decoy, hold=HOLD, after=None):
    """the call on a warm scanner on a gated stream, the producer of its input pending; returns (answer, scanner).
    after(sc, answer, which): checks of a route's diagnostics on every answer"""
    n = len(real.data)
    want = call(make(), real.ptr, n, None, real.lines)
    want_decoy = call(make(), decoy.ptr, n, None, decoy.lines)
    assert differ(want, want_decoy), "the decoy's answer does not differ from the real input's"
    assert guards_intact(want) and guards_intact(want_decoy)
    d_src = S.DeviceBuffer.from_bytes(decoy.data)
    s = GatedStream()
    try:
        sc = make()
        # the cold call makes every allocation (which may synchronise implicitly and hide a mistake)
        cold = call(sc, d_src.ptr, n, s.handle, decoy.lines)
        assert cold == want_decoy, "the cold call on the caller's stream"
        ref, seconds = timed(lambda: call(sc, d_src.ptr, n, None, decoy.lines))
        assert ref == want_decoy
        print("reference call: %.3f ms" % (seconds * 1e3))
        assert seconds < hold / 10, "the reference call takes %.2f ms: the gated call's issue may outlast the gate" % (seconds * 1e3)
        s.produce(d_src.ptr, real.ptr, n, hold)
        sc.probe = s.copy_pending       # asked after the outputs are allocated, straight before the library is entered
        got = call(sc, d_src.ptr, n, s.handle, real.lines)
        sc.probe = None
        returned, opened = sc.returned, s.opened_at
        assert sc.probed, "the gate was not closed when the call was made: the case is vacuous"
        assert got == want, "the call on a gated stream: %s" % (first_mismatch(got, want, want_decoy),)
        assert s.released.is_set() and opened is not None and opened <= returned, \
            "a synchronous call returned while its input was still gated"
        assert not s.timed_out
        assert guards_intact(got)
        if after:
            for which, answer in (("reference", want), ("cold", cold), ("gated", got)):
                after(sc, answer, which)
        return got, sc
    finally:
        s.close()
        d_src.free()


def first_mismatch(got, want, want_decoy):
    """which part of an answer differs, and whether it is the decoy's"""
    if got[0] != want[0]:
        return ("info", got[0], want[0], "the decoy's" if got[0] == want_decoy[0] else "")
    for k, (a, b) in enumerate(zip(got[1], want[1])):
        if a != b:
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            stale = k < len(want_decoy[1]) and a == want_decoy[1][k]
            return ("output", k, "first difference at", at, a[at:at + 8], b[at:at + 8], "the decoy's" if stale else "")
    return ("diagnostics", got[2], want[2])


@pytest.fixture(scope="module")
def kv(gpu):
    real, decoy = (Src(t) for t in kv_pair(21))
    yield real, decoy
    real.free()
    decoy.free()


# ------------------------------------------------------------------ a. every call kind

@pytest.mark.parametrize("name,make,call", CALLS, ids=CALL_IDS)
def test_every_call_kind_with_its_producer_pending(gpu, keys, kv, name, make, call):
    real, decoy = kv
    with S.Pool() as pool:
        got, sc = gated_check(lambda: make(pool, keys=keys), call, real, decoy)
        if name == "sort_lines":
            assert got[0].passes >= 2
        if name == "tally_top_lines":
            assert got[0].passes >= 2 and 40 <= got[0].nkeys <= 60
        assert sc.engine == S.ENGINE_SCAN
        if name != "scan":
            assert sc.last_lines_device == 1 and sc.last_line_batches == 1


# ------------------------------------------------------------------ b. the other routes

def five_calls(groups, vgroups, egroups):
    return [("scan_lines", call_scan_lines), ("filter_lines", call_filter), ("extract_lines", extract_call(egroups)),
            ("tally_sums_lines", sums_call(groups, vgroups)), ("tally_top_lines", top_call(groups, vgroups))]


KVW_CALLS = five_calls([1], [2, 3], [1, 2, 0])
OCTETS_CALLS = five_calls([2], [1, 2], [1, 2, 0])


@pytest.fixture(scope="module")
def dotted(gpu):
    real, decoy = (Src(t) for t in dotted_pair(2))
    yield real, decoy
    real.free()
    decoy.free()


@pytest.mark.parametrize("host", [0, 1], ids=["device", "host"])
@pytest.mark.parametrize("name,call", OCTETS_CALLS, ids=[c[0] for c in OCTETS_CALLS])
def test_the_nfa_tier_and_its_host_route(gpu, monkeypatch, dotted, name, call, host):
    real, decoy = dotted
    if host:
        monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")

    def after(sc, answer, which):
        assert sc.engine == S.ENGINE_NFA and answer[2][1] == 1 - host, (which, answer[2])

    with S.Pool() as pool:
        gated_check(lambda: kvw_scanner(pool, S.ENGINE_NFA, pats=OCTETS), call, real, decoy, after=after)


@pytest.mark.parametrize("name,call", KVW_CALLS, ids=[c[0] for c in KVW_CALLS])
def test_the_exact_vm(gpu, kv, name, call):
    real, decoy = kv

    def after(sc, answer, which):
        assert sc.engine == S.ENGINE_VM and answer[2][1] == 0, (which, answer[2])

    with S.Pool() as pool:
        gated_check(lambda: kvw_scanner(pool, S.ENGINE_VM), call, real, decoy, after=after)


@pytest.mark.parametrize("name,call", KVW_CALLS, ids=[c[0] for c in KVW_CALLS])
def test_several_batches(gpu, monkeypatch, kv, name, call):
    real, decoy = kv
    monkeypatch.setenv("SRE_HIP_LINES_BATCH", "64")

    def after(sc, answer, which):
        assert sc.engine == S.ENGINE_SCAN and answer[2][0] > 1 and answer[2][1] == 1, (which, answer[2])

    with S.Pool() as pool:
        gated_check(lambda: kvw_scanner(pool), call, real, decoy, after=after)


def test_find_all_rounds_on_the_nfa_tier(gpu, monkeypatch):
    """the find-all rounds that sre_hip_scan_results drives on the stream of the enqueue"""
    monkeypatch.setenv("SRE_HIP_COUNT_HORIZON", "256")
    real, decoy = (Src(t) for t in counted_pair(41))
    try:
        def after(sc, answer, which):
            assert sc.engine == S.ENGINE_NFA and answer[2][1] == 0, (which, answer[2])

        with S.Pool() as pool:
            got, _ = gated_check(lambda: kvw_scanner(pool, S.ENGINE_NFA, S.HIP_PIKE_COUNT, COUNTED), call_scan_lines, real, decoy,
                                 hold=FIND_ALL_HOLD, after=after)
            assert max(row[4] for row in got[1][0]) > 2, "no line with several matches"
    finally:
        real.free()
        decoy.free()


# ------------------------------------------------------------------ c. the asynchronous scan

def async_scan_check(make, real, decoy, ptrs_of, want_fixups=False):
    """enqueue on a gated stream returns while the gate is closed; results() then equal the null-stream scan's"""
    n = len(real)
    bufs = [S.DeviceBuffer.from_bytes(x) for x in (real, decoy, decoy)]
    s = GatedStream()
    try:
        d_real, d_decoy, d_src = (b.ptr for b in bufs)
        ref = make()
        want = ref.scan(*ptrs_of(d_real))
        if want_fixups:
            assert ref.last_fixups >= 1
        want_decoy = make().scan(*ptrs_of(d_decoy))
        assert want != want_decoy
        sc = make()
        assert sc.scan(*ptrs_of(d_src), s.handle) == want_decoy
        (_, seconds) = timed(lambda: sc.scan(*ptrs_of(d_src)))
        assert seconds < HOLD / 10, seconds
        s.produce(d_src, d_real, n)
        pending = s.copy_pending()
        sc.enqueue(*ptrs_of(d_src), s.handle)
        early = not s.released.is_set()
        got = sc.results()
        assert pending, "the gate was not closed when the scan was enqueued: the case is vacuous"
        assert early, "enqueue returned only after the gate had opened: it is not asynchronous"
        assert got == want
        assert s.released.is_set() and not s.timed_out
        if want_fixups:
            assert sc.last_fixups >= 1
        return sc
    finally:
        s.close()
        for b in bufs:
            b.free()


def whole(n):
    return lambda p: ([p], [n])


def test_enqueue_returns_while_the_stream_is_blocked(gpu, kv):
    real, decoy = kv
    spans = real.lines[:100]
    with S.Pool() as pool:
        sc = async_scan_check(lambda: kvw_scanner(pool), real.data, decoy.data,
                              lambda p: ([p + st for st, _ in spans], [k for _, k in spans]))
        assert sc.engine == S.ENGINE_SCAN


def test_enqueue_with_fixup_rounds_in_results(gpu, monkeypatch):
    """the subject of test_fixup_rounds_inside_a_set that defeats speculation: results() runs the rounds"""
    monkeypatch.setenv("SRE_HIP_SEG_BYTES", "256")
    real = b"xx a" + b"c" * 5000 + b"b" + b"c" * 3000
    decoy = b"c" * len(real)
    with S.Pool() as pool:
        sc = async_scan_check(lambda: kvw_scanner(pool, S.ENGINE_SCAN, pats=[rb"(?:a.*b|a)"]), real, decoy, whole(len(real)),
                              want_fixups=True)
        assert sc.engine == S.ENGINE_SCAN


@pytest.mark.parametrize("engine,pats", [(S.ENGINE_VM, KVW), (S.ENGINE_NFA, COUNTED)], ids=["vm", "nfa"])
def test_enqueue_on_the_other_engines(gpu, engine, pats):
    if engine == S.ENGINE_VM:
        real, decoy = kv_pair(23)
    else:
        real, decoy = counted_pair(43)
    spans = split_lines(real, 0x0A)[:100]
    with S.Pool() as pool:
        sc = async_scan_check(lambda: kvw_scanner(pool, engine, pats=pats), real, decoy,
                              lambda p: ([p + st for st, _ in spans], [k for _, k in spans]))
        assert sc.engine == engine


# ------------------------------------------------------------------ d. two scanners taking turns

def test_two_scanners_taking_turns_with_tail_streams(gpu, kv):
    """the header's recipe: the scans of A and B on their scan streams, what follows a scan on the tail streams, each
    scan ordered after the other scanner's; the results are collected one step late"""
    real, decoy = kv
    n = len(real.data)
    spans = decoy.lines[:120]           # one set of spans for every step's input

    def ptrs(p):
        return [p + st for st, _ in spans], [k for _, k in spans]

    inputs = [kv_text(50 + i, 4.4)[:n].ljust(n, b"#") for i in range(7)]
    assert len(set(inputs)) == 7 and all(len(x) == n for x in inputs)
    d_in = [S.DeviceBuffer.from_bytes(x) for x in inputs]
    d_src = [S.DeviceBuffer.from_bytes(decoy.data) for _ in range(2)]
    scan_streams, tail_streams = [GatedStream(), GatedStream()], [GatedStream(), GatedStream()]
    try:
        with S.Pool() as pool:
            ref = kvw_scanner(pool)
            wants = [ref.scan(*ptrs(b.ptr)) for b in d_in]
            want_decoy = ref.scan(*ptrs(decoy.ptr))
            # a step's buffer holds the decoy or the input of two steps before: a stale read of either cannot pass
            assert len({repr(w) for w in wants + [want_decoy]}) == 8
            _, seconds = timed(lambda: ref.scan(*ptrs(decoy.ptr)))
            print("reference scan: %.3f ms" % (seconds * 1e3))
            assert seconds < HOLD / 10, "the reference scan takes %.2f ms: an enqueue may outlast the gate" % (seconds * 1e3)
            scs = [kvw_scanner(pool), kvw_scanner(pool)]
            for i in range(2):
                scs[i].set_tail_stream(tail_streams[i].handle)
                assert scs[i].scan(*ptrs(d_src[i].ptr), scan_streams[i].handle) == want_decoy       # warm

            def gated_enqueue(i, step):
                """scanner i's scan of the step's input, which waits behind a closed gate when it is enqueued and when
                enqueue returns"""
                s = scan_streams[i]
                s.produce(d_src[i].ptr, d_in[step].ptr, n)
                pending = s.copy_pending()
                scs[i].enqueue(*ptrs(d_src[i].ptr), s.handle)
                early = not s.released.is_set()
                assert pending, ("step", step, "the gate was not closed when the scan was enqueued: the step is vacuous")
                assert early, ("step", step, "enqueue returned only after the gate had opened")

            for step in range(6):
                i = step % 2
                scs[1 - i].order_after_scan(scan_streams[i].handle)
                gated_enqueue(i, step)
                if step:
                    assert scs[1 - i].results() == wants[step - 1], ("step", step - 1)
            assert scs[1].results() == wants[5], ("step", 5)
            for sc in scs:
                sc.set_tail_stream(None)
            gated_enqueue(0, 6)
            assert scs[0].results() == wants[6], "without a tail stream"
            assert not any(s.timed_out for s in scan_streams)
    finally:
        for s in scan_streams + tail_streams:
            s.close()
        for b in d_in + d_src:
            b.free()


def test_a_line_call_ignores_the_tail_stream(gpu, kv):
    real, decoy = kv
    tail = GatedStream()
    try:
        with S.Pool() as pool:
            def make():
                sc = kvw_scanner(pool)
                sc.set_tail_stream(tail.handle)
                return sc
            gated_check(make, dict((c[0], c[2]) for c in CALLS)["tally_sums_lines"], real, decoy)
    finally:
        tail.close()


# ------------------------------------------------------------------ e. key sets and stream sets

@pytest.mark.parametrize("as_map", [False, True], ids=["set", "map"])
def test_a_key_set_created_on_a_gated_stream(gpu, kv, as_map):
    """create is synchronous on hip_stream and the set keeps its own copy of the rows"""
    real, _ = kv
    n = len(real.data)
    rows = dictionary_rows()[:60]
    other = [b"q" * len(k) for k in rows]               # no key of these is a key of the texts
    text, decoy_text = (map_text if as_map else set_text)(rows), (map_text if as_map else set_text)(other)
    assert len(text) == len(decoy_text) and not set(rows) & set(other)
    nfields, nkeys = (3, 1) if as_map else (1, None)
    d_rows, d_dict = S.DeviceBuffer.from_bytes(text), S.DeviceBuffer.from_bytes(decoy_text)
    s = GatedStream()
    made = []
    try:
        want_set = S.KeySet(d_rows.ptr, len(text), nfields, lib=gpu, nkeys=nkeys)
        made.append(want_set)
        (decoy_set, ref_seconds) = timed(lambda: S.KeySet(d_dict.ptr, len(text), nfields, lib=gpu, nkeys=nkeys))
        made.append(decoy_set)
        print("reference create: %.3f ms" % (ref_seconds * 1e3))
        assert ref_seconds < HOLD / 10, ref_seconds
        assert (want_set.rows, want_set.distinct) == (60, 60) and decoy_set.distinct < 60
        (warm, seconds) = timed(lambda: S.KeySet(d_dict.ptr, len(text), nfields, hip_stream=s.handle, lib=gpu, nkeys=nkeys))
        made.append(warm)
        assert seconds < HOLD / 10, seconds
        s.produce(d_dict.ptr, d_rows.ptr, len(text))
        pending = s.copy_pending()
        ks = S.KeySet(d_dict.ptr, len(text), nfields, hip_stream=s.handle, lib=gpu, nkeys=nkeys)
        made.append(ks)
        opened = s.released.is_set()
        assert gpu.sre_hip_upload(d_dict.ptr, bytes([FILL]) * len(text), len(text)) == 0
        assert pending, "the gate was not closed when the set was created: the case is vacuous"
        assert opened, "create returned while its rows were still gated"
        assert (ks.rows, ks.distinct, ks.values) == (want_set.rows, want_set.distinct, want_set.values)
        with S.Pool() as pool:
            sc = kvw_scanner(pool)
            call = call_join if as_map else call_lookup
            answers = []
            for which in (want_set, ks, decoy_set):
                sc.keys = Keys(which, which)
                answers.append(call(sc, real.ptr, n, None, real.lines))
            assert answers[1] == answers[0] and answers[2] != answers[0] and answers[0][0].nmembers > 0
    finally:
        s.close()
        for ks in made:
            ks.close()
        d_rows.free()
        d_dict.free()


PLANT = 9       # bytes of a planted match


def planted_streams(seed, nstreams, counted):
    """(subjects, decoys, schedules of three calls) whose records differ in every call by construction: a subject holds
    ONE match (of COUNTED, or of x(.*)y(.*)z), planted inside the chunk of call i % 3 of stream i, and its decoy holds one
    inside the chunk of the call after that one, so in either call one of the two matches and the other does not.  The
    chunks are those of test_gpu_streams.schedule, its first three calls"""
    rng = random.Random(seed)
    plant = b"abbbbbbb@" if counted else b"xaybbz\n  "[:PLANT]
    assert len(plant) == PLANT

    def base(n):
        if not counted:
            return bytearray(rng.choice(b"abyz \n") for _ in range(n))        # no x: no match
        text = bytearray(rng.choice(b"ab") for _ in range(n))
        for _ in range(n // 40):                                                # an @ that follows eight b: no match
            at = rng.randrange(0, n - PLANT)
            text[at:at + PLANT] = b"bbbbbbbb@"
        return text

    def matches(text):
        if not counted:
            return [i for i in range(len(text)) if text[i:i + 1] == b"x"]
        return [i - 8 for i in range(8, len(text)) if text[i] == 0x40 and text[i - 8] == 0x61 and b"@" not in text[i - 8:i]]

    subs, decoys, scheds, hits = [], [], [], [0, 0, 0]
    for i in range(nstreams):
        n = rng.choice([1000, 3000])
        while True:             # a schedule whose call i % 3 has room for the match
            sched = (schedule(rng, n) + [(0, 0, True)] * 3)[:3]
            if sched[i % 3][1] >= PLANT:
                break
        pair = []
        for call in (i % 3, (i + 1) % 3):
            off, size, _ = sched[call]
            text = base(n)
            at = off + rng.randrange(0, size - PLANT + 1) if size >= PLANT else n - PLANT
            text[at:at + PLANT] = plant
            assert matches(text) == [at]
            pair.append(bytes(text))
            # the stream is still open in that call: the real chunks hold no match before the call of their own
            hits[call] += i > 0 and size >= PLANT and call <= i % 3
        subs.append(pair[0])
        decoys.append(pair[1])
        scheds.append(sched)
    assert min(hits) >= nstreams // 3 - 1, hits         # (stream 0 starts again after every call and is not counted)
    return subs, decoys, scheds


@pytest.mark.parametrize("engine", [None, S.ENGINE_NFA], ids=["scan", "nfa"])
def test_a_stream_set_fed_on_a_gated_stream(gpu, engine):
    """24 streams, three calls of chunks, every call's chunks gated; stream 0 is reset between the calls.  Every call's
    records differ from what the decoy chunks would give in that call, and every reference feed is timed"""
    pats, mode = ([rb"x(.*)y(.*)z"], S.HIP_PIKE_FIRST) if engine is None else (COUNTED, S.HIP_THOMPSON)
    nstreams = 24
    hold = TABLE_SET_HOLD if engine is None else HOLD
    subs, decoys, scheds = planted_streams(61, nstreams, engine is not None)
    offs, o = [], 0
    for x in subs:
        offs.append(o)
        o += len(x)
    d_real, d_src = S.DeviceBuffer.from_bytes(b"".join(subs)), S.DeviceBuffer.from_bytes(b"".join(decoys))
    d_decoy = S.DeviceBuffer.from_bytes(b"".join(decoys))
    s = GatedStream()
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, pats))
            # want_set: the real chunks on the null stream; ss: the set under test; stale[k]: the real chunks up to call
            # k and the decoy's in call k, which is what a read of call k's chunks before their producer ran would give
            sets = [S.StreamSet(pool, prog, mode, nstreams, engine) for _ in range(5)]
            want_set, ss, stale = sets[0], sets[1], sets[2:]
            if engine is not None:
                assert ss.engine == S.ENGINE_NFA

            def args(base, k):
                return ([base + offs[i] + scheds[i][k][0] for i in range(nstreams)], [scheds[i][k][1] for i in range(nstreams)],
                        [scheds[i][k][2] for i in range(nstreams)])

            # the cold feeds, the three calls on the real and on the decoy chunks, make every allocation and load every
            # kernel; every stream starts again after them
            for t in sets:
                for base in (d_real.ptr, d_decoy.ptr):
                    for k in range(3):
                        t.feed(*args(base, k), s.handle if t is ss else None)
                    t.reset(range(nstreams))
            for k in range(3):
                want, seconds = timed(lambda: want_set.feed(*args(d_real.ptr, k)))
                print("reference feed %d: %.3f ms" % (k, seconds * 1e3))
                assert seconds < hold / 10, "the reference feed takes %.2f ms: the gated feed's issue may outlast the gate" % (seconds * 1e3)
                for t in stale[k + 1:]:
                    assert t.feed(*args(d_real.ptr, k)) == want
                want_stale = stale[k].feed(*args(d_decoy.ptr, k))
                assert want_stale != want, ("call", k, "the decoy chunks give the real chunks' records")
                assert gpu.sre_hip_upload(d_src.ptr, b"".join(decoys), o) == 0
                s.produce(d_src.ptr, d_real.ptr, o, hold)
                pending = s.copy_pending()
                got = ss.feed(*args(d_src.ptr, k), s.handle)
                opened = s.released.is_set()
                assert pending, "the gate was not closed when the chunks were fed: the case is vacuous"
                assert got == want, ("call", k, [i for i in range(nstreams) if got[i] != want[i]],
                                     "the decoy chunks' records" if got == want_stale else "")
                assert opened, "feed returned while its chunks were still gated"
                for t in sets:
                    t.reset([0])
            assert not s.timed_out
    finally:
        s.close()
        for b in (d_real, d_src, d_decoy):
            b.free()


def test_one_key_set_two_scanners_two_threads(gpu, keys, kv):
    """"any number of scanners and streams of the same device may use it at once": two host threads, each with its own
    scanner, stream and input, 20 lookups and joins each against the module's key set and key map"""
    texts = kv
    errors, answers = [], [[], []]
    with S.Pool() as pool:
        scs = [kvw_scanner(pool, keys=keys), kvw_scanner(pool, keys=keys)]
        serial = [(call_lookup(kvw_scanner(pool, keys=keys), t.ptr, len(t.data), None, t.lines),
                   call_join(kvw_scanner(pool, keys=keys), t.ptr, len(t.data), None, t.lines)) for t in texts]
        assert serial[0] != serial[1]
        streams = [GatedStream(), GatedStream()]
        start = threading.Barrier(2)

        def work(i):
            try:
                t = texts[i]
                start.wait(10)
                for _ in range(20):
                    answers[i].append((call_lookup(scs[i], t.ptr, len(t.data), streams[i].handle, t.lines),
                                       call_join(scs[i], t.ptr, len(t.data), streams[i].handle, t.lines)))
            except BaseException as e:      # (reported by the main thread)
                errors.append((i, repr(e)))

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        try:
            for t in threads:
                t.start()
            for t in threads:
                t.join(60)
        finally:
            for s in streams:
                s.close()
        assert not errors, errors
        for i in range(2):
            assert len(answers[i]) == 20
            assert all(a == serial[i] for a in answers[i]), (i, [k for k, a in enumerate(answers[i]) if a != serial[i]])
