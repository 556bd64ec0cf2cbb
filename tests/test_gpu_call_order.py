"""A call's answer does not depend on which call the scanner ran before.

Every call of a scanner builds its scan geometry from nothing (sre_hip_batch.cpp geom_device /
scan_geometry).  Each test runs a fixed sequence of different call kinds on ONE scanner and compares
every answer, and the diagnostics the other suites assert, with the same call on a scanner created
for it alone; the oracle checks of each call kind are in the suites of that kind.
"""
import os
import random

import pytest

import sregex_amd as S
from test_gpu_caller_stream import CALLS, CALL_IDS, Src, keys, kvw_scanner, line_cap      # noqa: F401 (keys: a fixture)
from test_gpu_lines import random_text, split_lines
from test_gpu_lines_tally_top import top_lines

pytestmark = pytest.mark.gpu

SHORT_MAX = 512         # sre_hip_lines.h SRE_LINES_SHORT_MAX
BATCH = 64              # lines per batch, forced: a line call has several batches


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


class Text:
    """about 300 lines on the device, one of them longer than the short-line limit"""

    def __init__(self, data):
        self.data = data
        self.lines = split_lines(data, 0x0A)
        assert 250 <= len(self.lines) <= 350 and len(self.lines) > 4 * BATCH
        assert sum(n > SHORT_MAX for _, n in self.lines) == 1
        self.buf = S.DeviceBuffer.from_bytes(data)

    def free(self):
        self.buf.free()


def scan_one(t):
    """the whole buffer as ONE stream"""
    return lambda sc: sc.scan([t.buf.ptr], [len(t.data)])


def scan_many(t):
    """every line as a stream"""
    return lambda sc: sc.scan([t.buf.ptr + st for st, _ in t.lines], [n for _, n in t.lines])


def scan_lines(t):
    def call(sc):
        got = sc.scan_lines(t.buf.ptr, len(t.data), all_lines=True, cap=len(t.lines) + 1)
        assert sc.last_line_batches > 1
        return got, sc.last_line_batches, sc.last_lines_device, sc.last_short_lines
    return call


def sink_call(t, run, index_words):
    """a line sink's call: its info, the output bytes and the index rows it wrote"""
    def call(sc):
        out = S.DeviceBuffer(2 * len(t.data) + 4 * len(t.lines) + 16)      # (an extracted row: at most twice its line)
        idx = S.DeviceBuffer(8 * index_words * len(t.lines))
        try:
            info = run(sc, out, idx)
            assert info.nlines == len(t.lines) and 0 < info.nselected == info.nwritten and sc.last_line_batches > 1
            return (info, out.to_bytes(info.out_bytes), idx.to_bytes(8 * index_words * info.nwritten), sc.last_line_batches,
                    sc.last_lines_device, sc.last_short_lines)
        finally:
            out.free()
            idx.free()
    return call


def filter_lines(t):
    return sink_call(t, lambda sc, out, idx: sc.filter_lines(t.buf.ptr, len(t.data), out.ptr, out.nbytes, index_ptr=idx.ptr,
                                                             index_cap=len(t.lines)), 4)


def extract_lines(t, groups):
    return sink_call(t, lambda sc, out, idx: sc.extract_lines(t.buf.ptr, len(t.data), groups, out.ptr, out.nbytes,
                                                              index_ptr=idx.ptr, index_cap=len(t.lines)), 4 + 2 * len(groups))


def run_sequence(make, steps):
    """the steps on one scanner, each compared with the same call on a fresh scanner; returns the answers"""
    sc = make()
    answers = []
    for k, (name, call) in enumerate(steps):
        got, want = call(sc), call(make())
        assert got == want, (k, name)
        answers.append(got)
    return answers


def test_table_driven_scanner(gpu, monkeypatch):
    monkeypatch.setenv("SRE_HIP_LINES_BATCH", str(BATCH))
    t = Text(random_text(31, nlines=300, nlong=1, long_bytes=(2048, 4096)))
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, [rb"([a-z]+)@([a-z]+)\.[a-z]+"]))

            def make():
                sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
                assert sc.engine == S.ENGINE_SCAN
                return sc

            one = ("scan of one stream", scan_one(t))
            answers = run_sequence(make, [one, ("scan_lines", scan_lines(t)), one, ("filter_lines", filter_lines(t)),
                                          ("scan of every line", scan_many(t)), ("extract_lines", extract_lines(t, [1, 2, 0])),
                                          one])
            assert answers[0] == answers[2] == answers[6] and answers[0][0][0] == 0
            assert answers[1][2] == 1                   # every batch on the device
            # the three line calls and the batch of streams agree on which lines match
            hits = [r[0] != S.SRE_DECLINED for r in answers[4]]
            assert [row[3] != S.SRE_DECLINED for row in answers[1][0][2]] == hits
            assert answers[3][0].nselected == answers[5][0].nselected == sum(hits) > 0
    finally:
        t.free()


def nfa_text(seed):
    rng = random.Random(seed)
    lines = [bytes(rng.choice(b"aaabbb@") for _ in range(rng.randrange(0, 200))) for _ in range(300)]
    lines.insert(137, bytes(rng.choice(b"aaabbb@") for _ in range(3000)))
    return b"\n".join(lines) + b"\n"


COUNTED = [rb"(?:a|b)*a(?:a|b){7}@"]


@pytest.mark.parametrize("mode", [S.HIP_PIKE_FIRST, S.HIP_THOMPSON])
def test_nfa_tier(gpu, monkeypatch, mode):
    monkeypatch.setenv("SRE_HIP_LINES_BATCH", str(BATCH))
    t = Text(nfa_text(37))
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, COUNTED))

            def make():
                sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
                assert sc.engine == S.ENGINE_NFA
                return sc

            lines = ("scan_lines", scan_lines(t))
            answers = run_sequence(make, [("scan of every line", scan_many(t)), lines, ("scan of one stream", scan_one(t)), lines])
            assert answers[1] == answers[3]
            (nl, nr, rows), _, device, nshort = answers[1]
            # the device route: the short-line kernel took every line but the long one, which has segments
            assert (nl, nr, device, nshort) == (len(t.lines), len(t.lines), 1, len(t.lines) - 1)
            assert [row[3:] for row in rows] == answers[0]
            assert 0 < sum(r[0] != S.SRE_DECLINED for r in answers[0]) < len(t.lines) and answers[2][0][0] == 0
    finally:
        t.free()


def test_nfa_tier_find_all(gpu, monkeypatch):
    """find-all rounds set per-stream flags and count requests; the line call between two of them takes the
    host route, which runs its batches through the same rounds"""
    monkeypatch.setenv("SRE_HIP_LINES_BATCH", str(BATCH))
    monkeypatch.setenv("SRE_HIP_COUNT_HORIZON", "256")
    t = Text(nfa_text(41))
    try:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, COUNTED))

            def make():
                sc = S.Scanner(pool, prog, S.HIP_PIKE_COUNT, S.ENGINE_NFA)
                assert sc.engine == S.ENGINE_NFA
                return sc

            def count(sc):
                # the long line and the lines in front of it
                spans = t.lines[:138]
                recs = sc.scan([t.buf.ptr + st for st, _ in spans], [n for _, n in spans])
                assert sc.last_count_rounds > 2
                return recs

            answers = run_sequence(make, [("find-all", count), ("scan_lines", scan_lines(t)), ("find-all", count)])
            assert answers[0] == answers[2]
            assert answers[1][2] == 0 and answers[1][3] == 0            # the host route
            # the line call and the batch of streams agree on every line's count
            (_, _, rows) = answers[1][0]
            assert [row[3:] for row in rows[:138]] == answers[0]
            assert rows[137][2] > SHORT_MAX and rows[137][4] > 2
    finally:
        t.free()


# ------------------------------------------------------------------ every kind after every other

@pytest.fixture(scope="module")
def order_texts(gpu, keys):
    """small: 60 lines (one batch); big: 2 101 lines over 1 025 keys (33 batches), the shapes of
    test_scratch_that_grows_inside_a_call_on_a_used_scanner: two workgroups of the values pass, three blocks of the entry
    table's scan, two digit passes; and the answer of every table call on each, from a scanner created for that call
    alone: 28 answers, computed once.  Every kind runs on a scanner of the KVW program here, route_lines with that
    program's one rule: the sinks that read capture groups cannot run on route_lines' own program, which has none"""
    saved = os.environ.get("SRE_HIP_LINES_BATCH")
    os.environ["SRE_HIP_LINES_BATCH"] = str(BATCH)
    texts = {"small": Src(top_lines(14, 20, miss=0)), "big": Src(top_lines(15, 1025, extra=1.05, span=300, miss=0))}
    try:
        assert len(texts["small"].lines) == 60 and len(texts["big"].lines) == 2101
        assert all(len(t.lines) <= line_cap(len(t.data)) for t in texts.values())
        fresh = {}
        with S.Pool() as pool:
            for name, _, call in CALLS:
                for size, t in texts.items():
                    fresh[name, size] = call(kvw_scanner(pool, keys=keys), t.ptr, len(t.data), None, t.lines)
                assert name == "scan" or fresh[name, "big"][2][0] > 1, "a line call of one batch"
                assert fresh[name, "small"] != fresh[name, "big"]
        assert fresh["tally_top_lines", "big"][0].nkeys == 1025 and fresh["tally_top_lines", "big"][0].passes >= 2
        assert fresh["sort_lines", "big"][0].passes >= 2
    except BaseException:
        for t in texts.values():
            t.free()
        raise
    finally:
        if saved is None:
            del os.environ["SRE_HIP_LINES_BATCH"]
        else:
            os.environ["SRE_HIP_LINES_BATCH"] = saved
    yield texts, fresh
    for t in texts.values():
        t.free()


@pytest.mark.parametrize("first", range(len(CALLS)), ids=CALL_IDS)
def test_every_line_call_after_every_other(gpu, monkeypatch, keys, order_texts, first):
    """A(small), B(big), A(small), B(small), A(big) on ONE scanner for every kind B: scratch that grows inside a call on
    a used scanner and is used again at the smaller size, and every ordered pair of kinds, all on the null stream"""
    monkeypatch.setenv("SRE_HIP_LINES_BATCH", str(BATCH))
    texts, fresh = order_texts
    name_a, _, call_a = CALLS[first]
    with S.Pool() as pool:
        sc = kvw_scanner(pool, keys=keys)
        for name_b, _, call_b in CALLS:
            steps = [(name_a, call_a, "small"), (name_b, call_b, "big"), (name_a, call_a, "small"), (name_b, call_b, "small"),
                     (name_a, call_a, "big")]
            for k, (name, call, size) in enumerate(steps):
                t = texts[size]
                got = call(sc, t.ptr, len(t.data), None, t.lines)
                assert got == fresh[name, size], "A = %s, B = %s, step %d: %s(%s) differs from a fresh scanner's" % (
                    name_a, name_b, k, name, size)
