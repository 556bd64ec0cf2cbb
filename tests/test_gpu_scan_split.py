"""The split walk of the scan kernel's common round (sre_hip_scan.hip "the split walk", sre_scan_split.h): the lookups of
a 64-byte round are walked as K sub-chains side by side, the chains behind the first from the guess that the lane is
still in the row it entered the round in; a wrong guess is walked again serially and makes the wave keep to the serial
walk for a number of rounds.

Every expected record comes from the oracle (_expect of tests/test_gpu_parity.py, as in tests/test_gpu_scan_forms.py);
ENGINE_SCAN is forced and the form each program runs on is asserted by name.  The subjects are a few hundred to 3000
bytes: the small geometry (256-byte segments: two warm-up rounds and four rounds each) unless a test sets another.
A round is 64 stream bytes from a multiple of 64, so with K = 2 the sub-chains meet at offset 32 of a round and with
K = 4 at 16, 32 and 48, whatever the class bits.  Which K a form is built with is scan_split_of's choice (K = 1 is
the serial walk; a library built with -DSRE_SCAN_SPLIT=2 or 4 splits in every form, and these tests hold for it as they
stand).  tests/test_scan_split_model.py checks the rule itself on the CPU.
"""
import pytest

import sregex_amd as S
import harness
from test_gpu_parity import _expect
from test_gpu_scan_forms import FORMS, compare, scanners, upload_all, MODES

pytestmark = pytest.mark.gpu

URI = FORMS[5][0][0]
# (regexes, class bits, FIRST / Thompson form, COUNT form, [(filler, event)]): a filler keeps the automaton in one state
# for whole rounds; an event is a single byte that changes the state or a whole match (with a growing tail for the GROW
# forms), or the end of the one long match the filler is.
PROGRAMS = [
    ([rb"[a-z]+"], 1, "sre_k_scan<1, 1, true, false>", "sre_k_scan<2, 1, true, true>",
     [(b" ", b"q"), (b" ", b"word"), (b"a", b" ")]),
    ([rb"\s+\S"], 1, "sre_k_scan<1, 1, true, false>", "sre_k_scan<2, 1, true, false>",
     [(b"a", b" "), (b"a", b"  b"), (b" ", b"a")]),
    ([rb"[a-z]+@[a-z]+\.[a-z]+"], 2, "sre_k_scan<1, 2, true, false>", "sre_k_scan<2, 2, true, true>",
     [(b"a", b"@"), (b" ", b"a@b.cde"), (b"a", b" "), (b"a", b"@b.c ")]),
    ([rb"\w+\s"], 2, "sre_k_scan<1, 2, true, false>", "sre_k_scan<2, 2, true, false>",
     [(b".", b"w"), (b".", b"w9 "), (b"a", b" ")]),
    ([URI], 4, "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, false, true>",
     [(b" ", b":"), (b"a", b" abc://abc.cc/ab/c?a=b "), (b"a", b"://b")]),
    ([rb"abcdefghij"], 4, "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, false, false>",
     [(b" ", b"a"), (b" ", b"abcdefghij"), (b" ", b"abcdefghi")]),
    ([rb"a+b+c+d+e+"], 4, "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, true, true>",
     [(b" ", b"a"), (b"a", b"bcdee"), (b" ", b"aabbccddeee"), (b"a", b" ")]),
    ([rb"abcd"], 4, "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, true, false>",
     [(b" ", b"a"), (b" ", b"abcd"), (b" ", b"abcabcd")]),
    ([rb"the quick brown fox"], 8, "sre_k_scan<1, 8, false, false>", "sre_k_scan<2, 8, false, false>",
     [(b" ", b"t"), (b"x", b"the quick brown fox"), (b" ", b"the quick ")]),
    ([rb"abcdefghijklmnopq+"], 8, "sre_k_scan<1, 8, false, false>", "sre_k_scan<2, 8, false, true>",
     [(b" ", b"a"), (b" ", b"abcdefghijklmnopqqq"), (b" ", b"abcdefghijklmnop")]),
]
IDS = ["%d-bit %s" % (p[1], p[0][0][:12].decode("latin-1")) for p in PROGRAMS]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def put(filler, n, events):
    """n bytes of filler with each event written over it at its offset"""
    out = bytearray(filler * n)
    for at, ev in events:
        out[at:at + len(ev)] = ev
    return bytes(out[:n])


def run(prog_row, datas, segs=(0,)):
    """every subject, each 0..3 bytes off alignment in a buffer of its own, in every mode against the oracle"""
    pats, bits, first_form, count_form, _ = prog_row
    ora = harness.OracleEngine()
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        scs = scanners(pool, prog)
        assert set(scs) == set(MODES), (pats, sorted(scs))
        for mode, sc in scs.items():
            want = count_form if mode == S.HIP_PIKE_COUNT else first_form
            assert sc.class_bits == bits and sc.kernel_name == want, (pats, mode, sc.class_bits, sc.kernel_name)
        expect = [_expect(ora, prog, re.ncaps, d) for d in datas]
        bufs, ptrs, lens = upload_all(datas, [i % 4 for i in range(len(datas))])
        try:
            for seg in segs:
                for mode, sc in scs.items():
                    sc.set_segment_bytes(seg)
                    got = sc.scan(ptrs, lens)
                    for i, (first, cnt) in enumerate(expect):
                        compare(got, mode, i, first, cnt, (pats, seg, len(datas[i]), i))
        finally:
            for b in bufs:
                b.free()
    return expect


@pytest.mark.parametrize("row", PROGRAMS, ids=IDS)
def test_hit_path(gpu, row):
    """Nothing but filler: every guess of every round hits.  Lengths around whole rounds and segments, ragged ends."""
    datas = [f * n for f in sorted({f for f, _ in row[4]}) for n in (256, 640, 1021, 1024, 1027, 2999)]
    run(row, datas)


@pytest.mark.parametrize("row", PROGRAMS, ids=IDS)
def test_one_event_at_every_offset_of_a_round(gpu, row):
    """One event in a stream of filler, beginning at stream offset 64 r + o for every o in 0..63 and r = 7 (a segment's
    last round) and 9 (the second round of the next): a miss in every sub-chain, an event on either side of every
    sub-chain boundary and across it, a match that leaves the fast path (FIRST) in the first and in a later chain, and
    in COUNT matches that end on the last byte of a chain and on the first byte of the next (a match of m bytes put at
    o ends at o + m - 1, and o takes every value), growing across the boundary in the GROW forms.  The ends are ragged."""
    datas = []
    for filler, ev in row[4]:
        for r in (7, 9):
            for o in range(64):
                datas.append(put(filler, 1024 + (o * 7) % 64, [(64 * r + o, ev)]))
    run(row, datas)


@pytest.mark.parametrize("row", PROGRAMS, ids=IDS)
def test_throttle_switches_on_and_off(gpu, row):
    """Quiet rounds and rounds with an event take turns at gaps of 1, 2, 3, 17 and 20 rounds: a miss makes the wave walk
    serially, the quiet stretch lets it split again, inside one segment (3000 bytes in one segment of 4096) and
    across the 256-byte segments of the small geometry; with two events in one round and events in neighbouring
    rounds."""
    datas = []
    for filler, ev in row[4]:
        for o in (0, 15, 16, 31, 32, 33, 48, 63):
            events, r = [], 2
            for gap in (1, 1, 17, 2, 20, 1, 3):
                if 64 * r + o + len(ev) >= 2990:
                    break
                events.append((64 * r + o, ev))
                r += gap
            events.append((64 * 2 + (o + 32) % 64, ev))
            datas.append(put(filler, 3000 - o % 5, events))
    run(row, datas, segs=(0, 4096))
