"""The edges of a row's readable range in the input staging (sre_hip_tile.h: tile_fetch of the table-driven scanner
and of the NFA tier's plain-slice kernel, tile2_fetch of the shift-and kernel).  A stage issues all four 16-byte loads
of a lane without a branch; a piece that does not lie wholly inside [lo, hi16 + 16) of its row is loaded from a block
of zeros instead, and the lane that owns those bytes reads them on the exact path.  That can only go wrong where a
range begins or ends, so the shapes are small: streams of 0 to 2049 bytes (small batches get 256-byte segments: one
segment, several, a ragged last piece, a last round shorter than 64 bytes, a row with nothing readable) starting at
every offset from a 16-byte boundary, with bytes around them that would change the answer if they were read.

Every expected value comes from the oracle (_expect of tests/test_gpu_parity.py); the engine is forced and the kernel
asserted by name.
"""
import os
import random

import pytest

import sregex_amd as S
import harness
from test_gpu_parity import _expect
from test_gpu_scan_forms import FORMS, MODES, compare, scanners, thompson_record

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("SRE_FUZZ_SEED", "0"))
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049)
HEADLINE = rb"[a-z]+@[a-z]+\.[a-z]+"
HEADLINE_GROUPS = rb"([a-z]+)@([a-z]+)\.([a-z]+)"
HEADLINE_PIECES = [b"a", b"bc", b"@", b".", b" ", b"a@b.c"]
HEADLINE_FIRST, HEADLINE_COUNT = "sre_k_scan<1, 2, true, false>", "sre_k_scan<2, 2, true, true>"
NFA_PAT = rb"(?:a|b)*a(?:a|b){7}@"
NFA_PIECES = [b"a", b"b", b"ab", b"@", b" ", b"abaabaabab@", b"abbbbbbb"]
# what lies between the streams: a match of its own wherever a kernel reads past a stream's ends
SCAN_FILL, NFA_FILL = b" q@q.q ", b" abaabaabab@ "
SEGMENT = 256       # what a small batch gets


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def place(datas, offsets, fill):
    """all subjects in one device buffer, subject i starting `offsets[i]` bytes past a 16-byte boundary, at least 32
    bytes of `fill` in front of, between and behind them"""
    blob, starts = bytearray(), []

    def pad(n):
        for _ in range(n):
            blob.append(fill[len(blob) % len(fill)])

    for d, o in zip(datas, offsets):
        pad(32)
        pad((o - len(blob)) % 16)
        starts.append(len(blob))
        blob.extend(d)
    pad(32)
    buf = S.DeviceBuffer.from_bytes(bytes(blob))
    assert buf.ptr % 16 == 0
    return buf, [buf.ptr + s for s in starts], [len(d) for d in datas]


def every_offset(rng, pieces):
    """(subjects, offsets): every length of LENGTHS at every offset 0..15, each subject a text of its own"""
    datas, offsets = [], []
    for n in LENGTHS:
        for o in range(16):
            out = bytearray()
            while len(out) < n:
                out += rng.choice(pieces)
            datas.append(bytes(out[:n]))
            offsets.append(o)
    return datas, offsets


def one_match(match, filler, back):
    """(subjects, offsets): every length of LENGTHS that holds `match`, the match as the only one of a text of
    `filler`: at byte 0, ending with the last byte, and `back` bytes in front of a 16-byte piece boundary, a 128-byte
    line boundary and a segment boundary, which it straddles"""
    datas, offsets, m = [], [], len(match)
    assert 0 < back < m <= 16
    for n in LENGTHS:
        for at in (0, n - m, 16 - back, 48 - back, 128 - back, SEGMENT - back, 2 * SEGMENT - back):
            if at < 0 or at + m > n:
                continue
            datas.append(filler * at + match + filler * (n - at - m))
            offsets.append((3 + 5 * len(datas)) % 16)
    return datas, offsets


def end_of_allocation(match, filler, fill):
    """[(buffer, pointer, subject)]: subjects that end with the last byte of their allocation, the last 16-byte piece
    of their rows partly outside, the only match ending with the subject's last byte"""
    out = []
    for n in (len(match), 77, 1003, 2049):
        d = filler * (n - len(match)) + match
        head = (fill * 4096)[:4096 - n]
        buf = S.DeviceBuffer.from_bytes(head + d)
        assert buf.nbytes == 4096 and n % 16 != 0
        out.append((buf, buf.ptr + 4096 - n, d))
    return out


def check_scan(pats, datas, offsets, fill, forms, segs=(0, 64), bufs=None):
    """every mode of the table-driven scanner on the subjects, each record against the oracle's"""
    ora = harness.OracleEngine()
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        scs = scanners(pool, prog)
        assert set(scs) == set(MODES), (pats, sorted(scs))
        if forms is not None:
            for mode, sc in scs.items():
                assert sc.kernel_name == forms[mode == S.HIP_PIKE_COUNT], (pats, mode, sc.kernel_name)
        expect = [_expect(ora, prog, re.ncaps, d) for d in datas]
        if bufs is None:
            buf, ptrs, lens = place(datas, offsets, fill)
            bufs = [buf]
        else:
            bufs, ptrs, lens = [b for b, _, _ in bufs], [p for _, p, _ in bufs], [len(d) for d in datas]
        for seg in segs:
            for mode, sc in scs.items():
                sc.set_segment_bytes(seg)
                got = sc.scan(ptrs, lens)
                for i, (first, cnt) in enumerate(expect):
                    compare(got, mode, i, first, cnt, (pats, seg, len(datas[i]), ptrs[i] % 16, datas[i][-80:]))
        for b in bufs:
            b.free()
        return expect


def check_nfa(datas, offsets, kernel, bufs=None):
    """Pike first-match and Thompson of NFA_PAT on the NFA tier, each record against the oracle's"""
    ora = harness.OracleEngine()
    with S.Pool() as pool:
        re = S.parse(pool, [NFA_PAT])
        prog = S.compile(pool, re)
        scs = {m: S.Scanner(pool, prog, m, S.ENGINE_NFA) for m in (S.HIP_THOMPSON, S.HIP_PIKE_FIRST)}
        for sc in scs.values():
            assert sc.engine == S.ENGINE_NFA and sc.kernel_name.startswith(kernel), sc.kernel_name
        expect = [_expect(ora, prog, re.ncaps, d)[0] for d in datas]
        if bufs is None:
            buf, ptrs, lens = place(datas, offsets, NFA_FILL)
            bufs = [buf]
        else:
            bufs, ptrs, lens = [b for b, _, _ in bufs], [p for _, p, _ in bufs], [len(d) for d in datas]
        for seg in (0, 64):
            for mode, sc in scs.items():
                sc.set_segment_bytes(seg)
                got = sc.scan(ptrs, lens)
                for i, first in enumerate(expect):
                    ctx = (kernel, seg, mode, len(datas[i]), ptrs[i] % 16, datas[i][-80:])
                    if mode == S.HIP_PIKE_FIRST:
                        assert got[i] == first, (ctx, got[i], first)
                    else:
                        assert got[i][:2] == thompson_record(first)[:2], (ctx, got[i], first)
        for b in bufs:
            b.free()
        return expect


# ------------------------------------------------------------------ the table-driven scanner (tile_fetch)

def test_headline_every_length_at_every_offset(gpu):
    """The headline program in its three modes on 320 streams in one batch: every length of LENGTHS at every offset
    0..15 from a 16-byte boundary."""
    datas, offsets = every_offset(random.Random(1601 + SEED), HEADLINE_PIECES)
    expect = check_scan([HEADLINE], datas, offsets, SCAN_FILL, (HEADLINE_FIRST, HEADLINE_COUNT))
    assert sum(first[0] >= 0 for first, _ in expect) > 100


@pytest.mark.parametrize("pat", [HEADLINE, HEADLINE_GROUPS], ids=["headline", "groups"])
def test_headline_only_match_at_the_edges(gpu, pat):
    """The only match of a stream at byte 0, at the last byte, across a piece, a line and a segment boundary: every
    slot of the record (with the three groups: eight of them) equals the oracle's."""
    datas, offsets = one_match(b"a@b.c", b" ", 2)
    expect = check_scan([pat], datas, offsets, SCAN_FILL, (HEADLINE_FIRST, HEADLINE_COUNT) if pat == HEADLINE else None)
    assert all(first[0] == 0 and cnt[1] == 1 for first, cnt in expect)
    assert len(expect) > 60


def test_headline_stream_at_the_end_of_its_allocation(gpu):
    """Streams cut from the very end of their allocation whose last 16-byte piece lies partly outside them: the piece
    is replaced by zeros, the exact path reads the tail byte by byte, and the match that ends with the last byte is
    found."""
    bufs = end_of_allocation(b"a@b.c", b" ", SCAN_FILL)
    expect = check_scan([HEADLINE_GROUPS], [d for _, _, d in bufs], None, None, None, bufs=bufs)
    assert all(first[0] == 0 for first, _ in expect)


@pytest.mark.parametrize("form,fill", [(FORMS[5], b" abc://abc.cc/ab/c?a=b "), (FORMS[10], b" the quick brown fox ")],
                         ids=["4-bit", "8-bit"])
def test_other_forms_every_length_at_every_offset(gpu, form, fill):
    """A 4-bit and an 8-bit form of the scan kernel (tile_store packs two classes into a byte, or copies the bytes)
    on the lengths and offsets of the first test."""
    pats, pieces, bits, first_form, count_form = form
    assert bits in (4, 8)
    datas, offsets = every_offset(random.Random(1600 + bits + SEED), pieces + [b"\x00", b"\xff"])
    check_scan(pats, datas, offsets, fill, (first_form, count_form), segs=(0,))


# ------------------------------------------------------------------ the NFA tier (tile2_fetch, tile_fetch)

@pytest.fixture(params=["sre_k_nfa_sa<", "sre_k_nfa<"], ids=["shift-and", "plain-slices"])
def nfa_kernel(request, monkeypatch):
    """the shift-and kernel (half-line staging, tile2_fetch) or, with the shift-and forms switched off (sre_nfa.h
    SRE_NFA_SA_*), the plain-slice kernel (tile_fetch)"""
    if request.param == "sre_k_nfa<":
        monkeypatch.setenv("SRE_HIP_NFA_SA", "128")
    return request.param


def test_nfa_every_length_at_every_offset(gpu, nfa_kernel):
    datas, offsets = every_offset(random.Random(1602 + SEED), NFA_PIECES)
    expect = check_nfa(datas, offsets, nfa_kernel)
    assert sum(first[0] >= 0 for first in expect) > 100


def test_nfa_only_match_at_the_edges(gpu, nfa_kernel):
    datas, offsets = one_match(b"abbabbab@", b" ", 4)
    expect = check_nfa(datas, offsets, nfa_kernel)
    assert all(first[0] == 0 for first in expect) and len(expect) > 60


def test_nfa_stream_at_the_end_of_its_allocation(gpu, nfa_kernel):
    bufs = end_of_allocation(b"abbabbab@", b" ", NFA_FILL)
    expect = check_nfa([d for _, _, d in bufs], None, nfa_kernel, bufs=bufs)
    assert all(first[0] == 0 for first in expect)
