"""The table-driven scanner, form by form (sre_hip_scan.hip scan_kernel_bits: sre_k_scan<MODE, BITS, WIDE, GROW>), and its
8-bit index form in particular: programs with more than 16 byte classes index the fast table with the input byte itself
(tile_store<8> copies raw bytes into the tile, sre_k_seg_functions<8> scales the byte, the capture walker's step16 takes
it as it is).  The generator's alphabet and the hand-written zoos of tests/test_gpu_parity.py stop at 4 bits.

Every expected value comes from the oracle (harness.OracleEngine through _expect of tests/test_gpu_parity.py, or fed the
same calls); ENGINE_SCAN is forced, so a decline raises; every form is asserted by name.  tests/test_scan_model.py
checks the host-built table of the same padded programs on the CPU: a failure here that it does not share is a kernel bug.
"""
import os
import random

import pytest

import sregex_amd as S
import harness
from harness import SCAN_PAD, pad_into_8bit_form, padded_subject
from test_gpu_lines import Expect, check, split_lines
from test_gpu_lines_filter import run_filter
from test_gpu_parity import _expect, _feed, record_fuzz_failures
from test_gpu_streams import CFG3, run_schedules, schedule

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("SRE_FUZZ_SEED", "0"))
URI = rb"([a-z]+)://([^/ ]+)(/[^ ?]*)?(\?[^ ]*)?"
MONTHS = rb"\b(january|february|march|april|june|july)\b"
STAMP = rb"(\d+)-(\d+)-(\d+)T(\d+):(\d+):(\d+)Z \[(info|warn|error)\]"
RANGES = rb"[a-c]+1|[d-f]+2|[g-i]+3|[j-l]+4|[m-o]+5|[p-r]+6|[s-u]+7|[v-x]+8|yz"
ALL_BYTES = rb"[0-9]+|[a-f]+|[g-m]+|[n-z]+|[A-Z]+|[\x80-\xbf]+|[\xc0-\xff]+|_|-|\.|,|;|:|!|\?|/|@"
# The pad's 17 bytes as single-byte alternatives: the same byte classes with one state instead of 17, for the two programs
# of section 4 that the builder declines with SCAN_PAD itself (every state of theirs times every position inside the
# pad's literal is more than the 62 rows of the fast table).
SINGLES = b"|" + b"|".join(bytes([c]) for c in SCAN_PAD[1:])
ROTATING_8BIT = rb"x(?:[^y]{3})*y" + SINGLES
MODES = (S.HIP_THOMPSON, S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT)

# every name scan_kernel_bits can return: FIRST / Thompson (MODE 1, never GROW) at 1, 2, 4 and 8 class bits (the tile
# is wide at 1 and 2 bits), COUNT (MODE 2) at 1, 2, 4 wide, 4 narrow and 8 bits, each with GROW and without
ALL_FORMS = {
    "sre_k_scan<1, 1, true, false>", "sre_k_scan<1, 2, true, false>", "sre_k_scan<1, 4, false, false>",
    "sre_k_scan<1, 8, false, false>",
    "sre_k_scan<2, 1, true, true>", "sre_k_scan<2, 1, true, false>",
    "sre_k_scan<2, 2, true, true>", "sre_k_scan<2, 2, true, false>",
    "sre_k_scan<2, 4, true, true>", "sre_k_scan<2, 4, true, false>",
    "sre_k_scan<2, 4, false, true>", "sre_k_scan<2, 4, false, false>",
    "sre_k_scan<2, 8, false, true>", "sre_k_scan<2, 8, false, false>",
}

# (regexes, pieces the subjects are made of beside 0x00 0x80 0xff, class bits, FIRST / Thompson form, COUNT form).
# A 4-bit COUNT table is wide while three workgroups still share a CU (sre_scan_tables_build: up to 9 states or so).
FORMS = [
    ([rb"x*"], [b"x", b"xx", b"y", b" "], 1, "sre_k_scan<1, 1, true, false>", "sre_k_scan<2, 1, true, true>"),
    ([rb"[a-z]+"], [b"a", b"zq", b" ", b"1", b"\n"], 1, "sre_k_scan<1, 1, true, false>", "sre_k_scan<2, 1, true, true>"),
    ([rb"\s+\S"], [b" ", b"\n", b"a", b"  ", b"#"], 1, "sre_k_scan<1, 1, true, false>", "sre_k_scan<2, 1, true, false>"),
    ([rb"[a-z]+@[a-z]+\.[a-z]+"], [b"a", b"bc", b"@", b".", b" ", b"a@b.c"], 2,
     "sre_k_scan<1, 2, true, false>", "sre_k_scan<2, 2, true, true>"),
    ([rb"\w+\s"], [b"a", b"_", b" ", b"\n", b".", b"w9"], 2, "sre_k_scan<1, 2, true, false>", "sre_k_scan<2, 2, true, false>"),
    ([URI], [b"abc", b"://", b"/", b"?", b" ", b"a=b", b"abc://abc.cc/ab/c?a=b ", b":", b"."], 4,
     "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, false, true>"),
    (CFG3, [b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"h", b"A", b"BLAH", b"BLA", b" ", b"\n", b"abcd", b"ef", b"#"], 4,
     "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, false, true>"),
    ([rb"abcdefghij"], [b"abcdefghij", b"abcde", b"abcdefghi", b"j", b"a", b" "], 4,
     "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, false, false>"),
    ([rb"a+b+c+d+e+"], [b"a", b"b", b"c", b"d", b"e", b"abcde", b"aabbccddee", b" "], 4,
     "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, true, true>"),
    ([rb"abcd"], [b"abcd", b"abc", b"a", b"b", b"c", b"d", b" "], 4,
     "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, true, false>"),
    ([rb"the quick brown fox"], [b"the quick brown fox", b"the quick ", b"brown fox", b"the ", b"t", b"x", b" "], 8,
     "sre_k_scan<1, 8, false, false>", "sre_k_scan<2, 8, false, false>"),
    ([rb"abcdefghijklmnopq+"], [b"abcdefghijklmnop", b"q", b"qqq", b"abcdefghijklmnopq", b"abcdefgh", b"a", b" "], 8,
     "sre_k_scan<1, 8, false, false>", "sre_k_scan<2, 8, false, true>"),
    ([RANGES], [b"a", b"bc", b"1", b"def", b"2", b"ghi3", b"k", b"4", b"mno5", b"q6", b"t", b"7", b"vwx8", b"yz", b"y", b" "], 8,
     "sre_k_scan<1, 8, false, false>", "sre_k_scan<2, 8, false, false>"),
    ([MONTHS], [b"january", b"february", b"march", b"april", b"june", b"july", b"jul", b"ju", b" ", b"_", b"y", b"\n", b"."], 8,
     "sre_k_scan<1, 8, false, false>", "sre_k_scan<2, 8, false, false>"),
    ([STAMP], [b"2026-10-18T19:21:00Z [info]", b"1-2-3T4:5:6Z [error]", b"12", b"-", b"T", b":", b"Z ", b"[warn]", b"[", b"]", b" "], 8,
     "sre_k_scan<1, 8, false, false>", "sre_k_scan<2, 8, false, false>"),
]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def thompson_record(first):
    """the Thompson record of a stream whose first-match record is `first`"""
    blank = [-1] * (len(first) - 2)
    return [0, 1] + blank if first[0] >= 0 else [S.SRE_DECLINED, 0] + blank


def upload_all(datas, offsets):
    """every subject in a device buffer of its own, `offset` bytes past the buffer's (aligned) start"""
    bufs = [S.DeviceBuffer.from_bytes(b"#" * o + d) for o, d in zip(offsets, datas)]
    return bufs, [b.ptr + o for b, o in zip(bufs, offsets)], [len(d) for d in datas]


def scanners(pool, prog, modes=MODES):
    """{mode: scanner} of the modes the table-driven scanner admits"""
    out = {}
    for mode in modes:
        try:
            out[mode] = S.Scanner(pool, prog, mode, S.ENGINE_SCAN)
        except RuntimeError:
            continue
    return out


def compare(got, mode, i, first, cnt, ctx):
    want = first if mode == S.HIP_PIKE_FIRST else cnt if mode == S.HIP_PIKE_COUNT else thompson_record(first)
    assert got[i] == want, (ctx, mode, i, got[i], want)


# ------------------------------------------------------------------ 1. every form, by name

def test_every_form_by_name_vs_oracle(gpu):
    """One program or more per instantiation of the scan kernel: the form it runs on is asserted literally, and the set
    of forms seen is the set scan_kernel_bits can return.  Subjects around the 64-byte round (0 to 3000 bytes and two
    longer ones made of runs) over the program's own bytes plus 0x00 0x80 0xff, each at another offset inside its
    buffer, with tiny and default segments, in every mode."""
    ora = harness.OracleEngine()
    rng = random.Random(8008 + SEED)
    seen = set()
    for pats, pieces, bits, first_form, count_form in FORMS:
        pieces = pieces + [b"\x00", b"\x80", b"\xff"]

        def text(n, runs=False):
            out = bytearray()
            while len(out) < n:
                out += rng.choice(pieces) * (rng.choice([1, 1, 2, 3, 9, 30, 70]) if runs else 1)
            return bytes(out[:n])

        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            scs = scanners(pool, prog)
            assert set(scs) == set(MODES), (pats, sorted(scs))
            for mode, sc in scs.items():
                want = count_form if mode == S.HIP_PIKE_COUNT else first_form
                assert sc.class_bits == bits and sc.kernel_name == want, (pats, mode, sc.class_bits, sc.kernel_name)
                seen.add(sc.kernel_name)
            datas = [text(n) for n in (0, 1, 63, 64, 65, 127, 128, 129, 200, 1000, 3000)] + [text(5000, True), text(9000, True)]
            expect = [_expect(ora, prog, re.ncaps, d) for d in datas]
            bufs, ptrs, lens = upload_all(datas, [(3 + 5 * i) % 16 for i in range(len(datas))])
            for seg in (64, 192, 4096, 0):
                for mode, sc in scs.items():
                    sc.set_segment_bytes(seg)
                    got = sc.scan(ptrs, lens)
                    for i, (first, cnt) in enumerate(expect):
                        compare(got, mode, i, first, cnt, (pats, seg, len(datas[i]), datas[i][:80]))
            for b in bufs:
                b.free()
    assert seen == ALL_FORMS, (sorted(ALL_FORMS - seen), sorted(seen - ALL_FORMS))


# ------------------------------------------------------------------ 2. all 256 byte values

# ALL_BYTES has 18 byte classes (the raw byte is the index); the others go through the class map (clsx) at 4, 2 and 1
# bits.  (The second and third have 4 and 2 classes, so they come out at 2 bits and at 1, not at 4 and 2: the first
# of the three was added for the 4-bit form.)
@pytest.mark.parametrize("pat,bits", [(ALL_BYTES, 8), (rb"[\x80-\xff]+|[a-z]+|\x00|[0-9]+|_", 4),
                                      (rb"[\x80-\xff]+|[a-z]+|\x00", 2), (rb"[\x80-\xff]+", 1)],
                         ids=["8-bit", "4-bit", "2-bit", "1-bit"])
def test_all_256_byte_values(gpu, pat, bits):
    """(a) uniformly random bytes over all 256 values; (b) 256 streams in one call, stream v a filler no class of the
    program matches with byte v at offset 100, inside a full round: the record of every v equals the oracle's (a
    signedness slip on bytes of 0x80 and above, a real NUL beside the zeros the tile reads outside a row)."""
    ora = harness.OracleEngine()
    rng = random.Random(256 + bits + SEED)
    with S.Pool() as pool:
        re = S.parse(pool, [pat])
        prog = S.compile(pool, re)
        scs = scanners(pool, prog, (S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT))
        assert set(scs) == {S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT}
        for sc in scs.values():
            assert sc.class_bits == bits, (pat, sc.class_bits)
        datas = [bytes(rng.randrange(256) for _ in range(n)) for n in (64, 65, 127, 129, 500, 1000, 2500, 4000)]
        bufs, ptrs, lens = upload_all(datas, [(7 + 3 * i) % 16 for i in range(len(datas))])
        streams = [b"#" * 100 + bytes([v]) + b"#" * 99 for v in range(256)]
        blob = S.DeviceBuffer.from_bytes(b"#" * 5 + b"".join(streams))
        datas += streams
        ptrs += [blob.ptr + 5 + 200 * v for v in range(256)]
        lens += [200] * 256
        expect = [_expect(ora, prog, re.ncaps, d) for d in datas]
        assert len({tuple(first) for first, _ in expect[-256:]}) == 2       # the one byte decides: a match or none
        for seg in (64, 0):
            for mode, sc in scs.items():
                sc.set_segment_bytes(seg)
                got = sc.scan(ptrs, lens)
                for i, (first, cnt) in enumerate(expect):
                    compare(got, mode, i, first, cnt, (pat, seg, len(datas[i]), datas[i][96:104]))
        for b in bufs + [blob]:
            b.free()


# ------------------------------------------------------------------ 3. random programs in the 8-bit form

@pytest.mark.parametrize("seg", [64, 0])
def test_padded_random_patterns_vs_oracle(gpu, seg):
    """The programs of test_scanner_random_patterns_vs_oracle with SCAN_PAD appended to their first regex, which lifts
    them over 16 byte classes; its subjects (and 1500 bytes), half of them with the pad's literal, a prefix of it or one
    of 0x00 0x80 0xff inserted.  Every mode the scanner admits against the oracle; failing cases go to
    the log of test_scanner_random_patterns_vs_oracle, which tools/fuzz_repro.py --file replays.  At least three programs in four must run in the 8-bit form
    (on the CPU 530 of 600 do; the others exceed the builder's state cap)."""
    ora = harness.OracleEngine()
    rng = random.Random(20261004 + SEED + seg + 8)
    programs, eight, bad = 150, 0, []
    for _ in range(programs):
        nre = 1 if rng.random() < 0.8 else rng.randrange(2, 4)
        pats = pad_into_8bit_form([harness.random_regex(rng) for _ in range(nre)])
        datas = [padded_subject(rng, rng.choice([0, 1, 7, 64, 65, 130, 400, 1500])) for _ in range(6)]
        offs = [rng.randrange(0, 16) for _ in datas]
        with S.Pool() as pool:
            try:
                re = S.parse(pool, pats)
            except Exception:
                continue
            prog = S.compile(pool, re)
            scs = scanners(pool, prog)
            if S.HIP_PIKE_FIRST not in scs:
                continue        # the builder declines the program (its state cap, a look-ahead it does not take)
            eight += scs[S.HIP_PIKE_FIRST].class_bits == 8
            bufs, ptrs, lens = upload_all(datas, offs)
            got = {}
            for mode, sc in scs.items():
                if seg:
                    sc.set_segment_bytes(seg)
                got[mode] = sc.scan(ptrs, lens)
            for i, d in enumerate(datas):
                first, cnt = _expect(ora, prog, re.ncaps, d)
                t = ora.thompson(prog)
                th = t.exec(d, True)
                t.close()
                for mode, recs in got.items():
                    want = first if mode == S.HIP_PIKE_FIRST else cnt if mode == S.HIP_PIKE_COUNT else None
                    if want is None and th == S.SRE_ERROR:
                        continue            # the reference's Thompson list overflows here (oracle guard)
                    if not (recs[i][0] == th if want is None else recs[i] == want):
                        bad.append({"engine": "scan", "mode": mode, "seg": seg, "re": [p.hex() for p in pats],
                                    "s": d.hex(), "got": recs[i], "want": want if want is not None else [th]})
            for b in bufs:
                b.free()
    record_fuzz_failures(bad)
    print("padded programs admitted in the 8-bit form: %d of %d (seg %d)" % (eight, programs, seg))
    assert not bad, (len(bad), [(b["mode"], bytes.fromhex(b["re"][0]), b["s"][:40], b["got"][:4], b["want"][:4]) for b in bad[:6]])
    assert eight >= 0.75 * programs, (eight, programs)


# ------------------------------------------------------------------ 4. the slow paths of the 8-bit form

def eight_bit(pool, prog, mode, seg):
    sc = S.Scanner(pool, prog, mode, S.ENGINE_SCAN)
    assert sc.class_bits == 8, sc.class_bits
    sc.set_segment_bytes(seg)
    return sc


def test_8bit_fixup_rounds_are_reported(gpu):
    """test_scanner_fixup_rounds_are_reported in the 8-bit form.  (0xe2 is 'b' with the top bit set: a match that
    reaches it took the byte for a 'b'.)"""
    ora = harness.OracleEngine()
    with S.Pool() as pool:
        re = S.parse(pool, pad_into_8bit_form([rb"(?:a.*b|a)"]))
        prog = S.compile(pool, re)
        sc = eight_bit(pool, prog, S.HIP_PIKE_FIRST, 64)
        data = b"xx a" + b"c" * 500 + b"b" + b"c" * 100 + b"\xe2" + b"c" * 199
        first, _ = _expect(ora, prog, re.ncaps, data)
        assert first == [0, 1, 3, 505]
        buf = S.DeviceBuffer.from_bytes(data)
        rec = sc.scan([buf.ptr], [len(data)])[0]
        buf.free()
        assert rec == first
        assert sc.last_fixups >= 1


def test_8bit_automaton_that_never_forgets_gets_exact_entry_states(gpu):
    """test_scanner_automaton_that_never_forgets_gets_exact_entry_states in the 8-bit form, 3000 periods instead of
    20000: the state rotates with the input, speculation fails, and after two rounds sre_k_seg_functions<8> composes
    the segments' transition functions (last_exact_passes is the only proof that it ran).  x(?:[^y]{3})*y padded with
    SCAN_PAD is beyond the builder's state cap, so it runs as ROTATING_8BIT.  Every 50th period holds 0xf8 ('x' with
    the top bit set) where its 'a' was: the rotation goes on over it, while an 'x' there would list a second thread."""
    ora = harness.OracleEngine()
    with S.Pool() as pool:
        with pytest.raises(RuntimeError):
            S.Scanner(pool, S.compile(pool, S.parse(pool, pad_into_8bit_form([rb"x(?:[^y]{3})*y"]))), S.HIP_PIKE_FIRST,
                      S.ENGINE_SCAN)
    body = (b"abc" * 49 + b"\xf8bc") * 60
    cases = [([ROTATING_8BIT], b"ab" * 50 + b"x" + body + b"ab" + b"y" + b"zz"),
             ([ROTATING_8BIT], b"x" + body + b"y" + b"zz"),
             (pad_into_8bit_form([rb"(a)(?:[bc]{2})*(d)"]), b"q" * 777 + b"a" + b"bc" * 3001 + b"bd" + b"bc" * 500)]
    for seg in (256, 1280):
        for pats, data in cases:
            with S.Pool() as pool:
                re = S.parse(pool, pats)
                prog = S.compile(pool, re)
                first, _ = _expect(ora, prog, re.ncaps, data)
                buf = S.DeviceBuffer.from_bytes(data)
                for mode, want in ((S.HIP_PIKE_FIRST, first), (S.HIP_THOMPSON, thompson_record(first))):
                    sc = eight_bit(pool, prog, mode, seg)
                    rec = sc.scan([buf.ptr], [len(data)])[0]
                    assert rec == want, (pats, seg, mode, rec, want)
                    assert sc.last_fixups <= 4, (pats, seg, mode, sc.last_fixups)
                    assert sc.last_exact_passes >= 1, (pats, seg, mode, sc.last_fixups)
                buf.free()


def test_8bit_count_automaton_that_never_forgets_gets_exact_entry_states(gpu):
    """test_count_automaton_that_never_forgets_gets_exact_entry_states in the 8-bit form, about 2500 quoted words
    instead of 9000: COUNT composes the segments' functions too (sre_k_seg_functions<8> with the caller's restarts).
    0xa2 is '"' with the top bit set; it stands outside the strings, where a quote would open one.  The two-regex program
    padded with SCAN_PAD is beyond the builder's state cap and runs with SINGLES.  The last case settles by
    speculation (the 128 bytes of warm-up in front of a segment hold an 'x'): it checks the record and the fix-up bound
    only, the other five prove that the exact pass ran."""
    ora = harness.OracleEngine()
    rng = random.Random(11 + SEED)
    words = [b'"ab" cde ', b'"abc" "d" e', b'"" x', b'key\xa2: "va lue", ', b"'q' ", b"\xa2 \x00 "]
    text = b"".join(rng.choice(words) for _ in range(2500))
    quoted = pad_into_8bit_form([rb'"[^"]*"'])
    with S.Pool() as pool:
        with pytest.raises(RuntimeError):
            S.Scanner(pool, S.compile(pool, S.parse(pool, pad_into_8bit_form([rb'"[^"]*"', rb"'[^']*'"]))), S.HIP_PIKE_COUNT,
                      S.ENGINE_SCAN)
    # (the last one settles by speculation: the 128 bytes of warm-up in front of a segment hold an 'x')
    cases = [(quoted, b'"ab" cde\xa2' * 2500, True), (quoted, b'"abc" "d" e' * 2000, True), (quoted, text, True),
             (pad_into_8bit_form([rb'"([^"]*)"']), text, True), ([rb'"[^"]*"' + SINGLES, rb"'[^']*'"], text, True),
             ([ROTATING_8BIT], b"x\xf8bcabcy z" * 2500, False)]
    for seg in (256, 1280):
        for pats, data, parity in cases:
            with S.Pool() as pool:
                re = S.parse(pool, pats)
                prog = S.compile(pool, re)
                _, cnt = _expect(ora, prog, re.ncaps, data)
                buf = S.DeviceBuffer.from_bytes(data)
                sc = eight_bit(pool, prog, S.HIP_PIKE_COUNT, seg)
                rec = sc.scan([buf.ptr], [len(data)])[0]
                buf.free()
                assert rec == cnt, (pats, seg, rec, cnt)
                assert sc.last_fixups <= 12, (pats, seg, sc.last_fixups)
                assert not parity or sc.last_exact_passes >= 1, (pats, seg, sc.last_fixups)


@pytest.mark.parametrize("seg", [64, 4096])
def test_8bit_long_lineage_uses_ancestor_maps(gpu, seg):
    """test_scanner_long_lineage_uses_ancestor_maps in the 8-bit form on 20000-byte subjects: the capture walker replays
    long stretches through the packed fast table, 16 bytes a load (Tracer::step16, the byte itself as the index; the
    subjects start at a 16-byte boundary, which that path asks for).  0xf8 0xf9 0xfa are x y z with the top bit set: a
    0xf9 in the first run taken for a 'y' moves the automaton to another state."""
    ora = harness.OracleEngine()
    rng = random.Random(16 + SEED)

    def run(pair, n):
        out = bytearray(pair * (n // 2))
        for at in range(40, len(out), 97):
            out[at] = rng.choice(b"\xf8\xf9\xfa\x00\x80\xff")
        return bytes(out)

    cases = [
        (pad_into_8bit_form([rb"x(.*)y(.*)z"]), b"..x" + run(b"ab", 13000) + b"y" + run(b"cd", 6990) + b"z.."),
        (pad_into_8bit_form([rb"([a-z]+)@([a-z]+)\.([a-z]+)"]), S.gen_data_host(20000, b"@abc.cc ")),
        (pad_into_8bit_form([rb"(a|b|c)+(@)(x)?"]), S.gen_data_host(20003, b"@")),
        # a group inside the loop saves a slot with every byte: no stretch of it is stable, the walk to the 'x' goes
        # byte by byte and replays every block it enters
        (pad_into_8bit_form([rb"x(.)*y(.*)z"]), b"..x" + run(b"ab", 13000) + b"y" + run(b"cd", 6990) + b"z.."),
        # ... and here a 'k' takes a thread out of the list in front of the one the walk follows (0xeb is 'k' with the
        # top bit set): a replay that takes the 0xeb for a 'k' hands the walk a state with that thread at another place.
        # (SINGLES: with SCAN_PAD itself the program is beyond the builder's state cap.)
        ([rb"x(?:[^k]*(?:k[^k]*)?!|(.)*z)" + SINGLES], b"..x" + run(b"ab", 19990).replace(b"\xf9", b"\xeb") + b"z.."),
    ]
    passes = []
    for pats, data in cases:
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            first, cnt = _expect(ora, prog, re.ncaps, data)
            assert first[0] == 0 and first[3] - first[2] > 19000, (pats, first)
            buf = S.DeviceBuffer.from_bytes(data)
            assert buf.ptr % 16 == 0
            other = S.DeviceBuffer.from_bytes(b"zz a@b.c zz")
            sc = eight_bit(pool, prog, S.HIP_PIKE_FIRST, seg)
            recs = sc.scan([other.ptr, buf.ptr, buf.ptr], [11, len(data), len(data)])
            assert recs[1] == first and recs[2] == first, (pats, seg, recs[1], first)
            passes.append(sc.last_lineage_passes)
            sc2 = eight_bit(pool, prog, S.HIP_PIKE_COUNT, seg)
            assert sc2.scan([buf.ptr], [len(data)])[0] == cnt, (pats, seg)
            buf.free()
            other.free()
    # the thread list of the third case changes with every byte: it must take the ancestor maps
    assert passes[2] == 1, passes


# ------------------------------------------------------------------ 5. the other entry points of the same kernel

def log_lines(rng, n, hit=1 / 3):
    """n log lines without their newlines; about `hit` of them hold a full STAMP match, some hold 0x00 and 0xff"""
    levels = [b"info", b"warn", b"error"]
    out = []
    for _ in range(n):
        stamp = b"%d-%02d-%02dT%02d:%02d:%02dZ" % (rng.randrange(1990, 2030), rng.randrange(1, 13), rng.randrange(1, 29),
                                                   rng.randrange(24), rng.randrange(60), rng.randrange(60))
        r = rng.random()
        if r < hit:
            line = stamp + b" [" + rng.choice(levels) + b"]"
        elif r < hit + 0.2:
            line = stamp + b" [" + rng.choice([b"debug", b"inf", b"warn ", b"\xff", b"\x00info"]) + b"]"
        elif r < hit + 0.4:
            line = stamp[:rng.randrange(0, len(stamp))] + rng.choice([b"", b"\x00", b"\xff", b"\x80"])
        else:
            line = b""
        words = [b"started", b"worker 7", b"\x00", b"\xff\xfe", b"took 12:30", b"[info", b"-", b"Z [", b"caf\xc3\xa9"]
        head = b" ".join(rng.choice(words) for _ in range(rng.randrange(0, 3)))
        tail = b" ".join(rng.choice(words) for _ in range(rng.randrange(0, 4)))
        out.append(head + (b" " if head else b"") + line + (b" " if tail else b"") + tail)
    return out


def stamp_program(pool):
    re = S.parse(pool, [STAMP])
    prog = S.compile(pool, re)
    for mode in MODES:
        assert S.Scanner(pool, prog, mode, S.ENGINE_SCAN).class_bits == 8
    return re, prog


@pytest.mark.parametrize("mode", [S.HIP_PIKE_FIRST, S.HIP_THOMPSON])
def test_8bit_stream_set_vs_oracle(gpu, mode):
    """A stream set of an 8-bit program with 7 groups: 32 streams with their own chunk schedules, every call of every
    stream against the oracle fed the same call."""
    rng = random.Random(3232 + SEED + mode)
    with S.Pool() as pool:
        re, prog = stamp_program(pool)
        subs = []
        for i in range(32):
            # the match early, late or (every fourth stream) nowhere
            lines = log_lines(rng, rng.choice([8, 120, 500]), hit=0.0 if i % 4 == 3 else rng.choice([0.02, 0.3]))
            subs.append(b"\n".join(lines))
        scheds = [schedule(rng, len(s)) for s in subs]
        n = run_schedules(gpu, pool, prog, re.ncaps, mode, subs, scheds, rng, engine=S.ENGINE_SCAN)
        assert n == sum(map(len, scheds))


def test_8bit_line_mode_and_filter_vs_oracle(gpu):
    """Line mode and the line filter on an 8-bit program: 3000 log lines, a third of them matching, some with 0x00 and
    0xff; rows and the filtered buffer against the oracle line by line."""
    rng = random.Random(3000 + SEED)
    lines = log_lines(rng, 3000)
    data = b"\n".join(lines) + b"\n"
    assert b"\x00" in data and b"\xff" in data
    with S.Pool() as pool:
        re, prog = stamp_program(pool)
        exp = Expect(prog, re.ncaps)
        hits = sum(exp.record(ln, S.HIP_PIKE_FIRST)[0] >= 0 for ln in lines)
        assert 800 < hits < 1200, hits
        assert len(split_lines(data, 0x0A)) == 3000
        for mode in MODES:
            sc = S.Scanner(pool, prog, mode, S.ENGINE_SCAN)
            assert sc.class_bits == 8
            for all_lines in (False, True):
                check(sc, exp, data, 0x0A, mode, all_lines, offset=5)
            run_filter(sc, exp, data, 0x0A, mode, src_off=3, dst_off=1)
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST, S.ENGINE_SCAN)
        run_filter(sc, exp, data, 0x0A, S.HIP_PIKE_FIRST, invert=True)


def test_8bit_compat_api_chunked_streams_take_the_scanner(gpu):
    """sre_vm_pike_exec fed an 8-bit program in chunks large enough for the scanner (one schedule starts with 100 KiB):
    every call answers what the oracle answers to the same call, and none of them runs on the exact VM."""
    ora = harness.OracleEngine()
    eng = harness.ProductEngine()
    rng = random.Random(100 + SEED)
    with S.Pool() as pool:
        re, prog = stamp_program(pool)
        nov = 2 * (re.ncaps + 1)
        miss = b"\n".join(log_lines(rng, 10000, hit=0.0)) + b"\n"
        assert len(miss) > 200000
        hit = b"1999-12-31T23:59:59Z [warn] \x00\xff\n"
        for data, sizes in ((miss + hit + miss[:5000], [100 << 10, 4096, 1, 50000]),
                            (miss[:30000] + hit + miss[:100], [4096, 4096, 10000]),
                            (miss[:150000], [5000, 70000, 0, 4097])):
            want = _feed(ora.pike(prog, re.ncaps), data, sizes, nov)
            before = S.compat_route_counts()
            got = _feed(eng.pike(prog, re.ncaps), data, sizes, nov)
            after = S.compat_route_counts()
            assert got == want, (len(data), sizes, got[-2:], want[-2:])
            assert len(got) > 2
            assert after[2] == before[2], (before, after)
            assert after[1] - before[1] == len(got), (before, after, len(got))
            eng.recycle()
    eng.pool.destroy()
