"""The line sort by text (sre_hip_sort_lines_text) on the device against pure Python: the oracle's first-match field of the sort
group per line, cut at max_bytes, and Python's stable sorted() on those bytes (reverse=True keeps ties in line order, as the
call does); the lines without a match follow in line order under ALL; limit is a slice.  Output and index buffers carry guard
bytes and a fill.  Every call's info.passes is checked against len(S.sort_text_plan(minlen, maxlen, rest)).  Unless a case opts
out the runner asserts of its INPUT that an unsorted or unstable output could not pass: not already in output order, and two
equal compared texts with a different one between them."""
import random

import pytest

import sregex_amd as S
from hipstream import GatedStream
from test_gpu_lines import split_lines, upload_at
from test_gpu_lines_filter import Out, run_filter
from test_gpu_lines_extract import Program, expected
from test_gpu_lines_tally import words
from test_gpu_lines_sort import run_sort

pytestmark = pytest.mark.gpu

N = 3000                # three workgroups of the values pass, several partition slots
SIZE_MAX = (1 << 64) - 1
K = [rb"k=([^ ]*)"]
# group 1 unset for a line that only has "u="
KU = [rb"(?:k=([^ ]*)|u=)"]
# two columns: text and number
AB = [rb"a=([^ ]*) b=([^ ]*) n=(-?[0-9]*)"]
# a counted repeat around the group, for the NFA tier
COUNTED = [rb"t=[0-9]{1,3}ms k=([a-z.]{0,12})"]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def expect(exp, data, group, max_bytes, desc, all_lines, delim=0x0A):
    """(field per line: (offset, length), "unset" or None; compared text per keyed line; [(line, start, len)] in output order)"""
    lines = split_lines(data, delim)
    field, cut = [None] * len(lines), {}
    for i, _, _, fl in expected(exp, data, delim, [group], False):
        field[i] = fl[0] if fl[0] else "unset"
        t = data[fl[0][0]:fl[0][0] + fl[0][1]] if fl[0] else b""
        cut[i] = t[:max_bytes] if max_bytes else t
    keyed = sorted(cut, key=lambda i: cut[i], reverse=desc)        # (sorted(cut) walks the lines in line order: dicts keep it)
    rest = [i for i in range(len(lines)) if field[i] is None] if all_lines else []
    return field, cut, [(i,) + lines[i] for i in keyed + rest]


def shape_holds(cut, cand):
    texts = [cut[i] for i in sorted(cut)]
    order = [r[0] for r in cand]
    last, between = {}, False
    for at, t in enumerate(texts):
        if t in last and any(w != t for w in texts[last[t] + 1:at]):
            between = True
        last[t] = at
    return order != sorted(order) and between


def run_text(sc, exp, data, group=1, max_bytes=0, desc=False, all_lines=False, limit=0, delim=0x0A, src_off=0, dst_off=0,
             out_cap=None, index_cap=None, null_out=False, shape=True, stream=None, src_ptr=None):
    """one call, checked in full; returns (info, output bytes, index rows).  src_ptr: the data is on the device already"""
    lib = sc.lib
    d = bytes([delim])
    field, cut, cand = expect(exp, data, group, max_bytes, desc, all_lines, delim)
    nlines = len(field)
    if shape and len(cand) >= 4:
        assert shape_holds(cut, cand), "the case's input does not exercise the sort"
    lens = [len(t) for t in cut.values()]
    minlen, maxlen = min(lens, default=SIZE_MAX), max(lens, default=0)
    plan = S.sort_text_plan(minlen, maxlen, all_lines and len(cut) < nlines)
    sel = cand[:limit] if limit else cand
    need = sum(n + 1 for _, _, n in sel)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for _, _, n in sel:
        if out_bytes + n + 1 > cap:
            break
        out_bytes += n + 1
        nwritten += 1
    want = b"".join(data[st:st + n] + d for _, st, n in sel[:nwritten])
    icap = len(sel) + 3 if index_cap is None else index_cap
    src = upload_at(data, src_off) if src_ptr is None else None
    out, idx = Out(lib, cap, dst_off), Out(lib, icap * 48, 0)
    try:
        info = sc.sort_lines_text(src.ptr + src_off if src else src_ptr, len(data), None if null_out else out.ptr, cap, group, delim,
                                  max_bytes, desc, all_lines, limit, idx.ptr if icap else None, icap, stream)
        want_info = S.SortTextInfo(nlines, len(cut), len(sel), need, nwritten, out_bytes, len(plan), minlen, maxlen)
        print("sort_lines_text", nlines, "lines:", info)
        assert info == want_info, (info, want_info)
        out.check(want)
        nidx = min(icap, nwritten)
        rows, o = [], 0
        for i, st, n in sel[:nidx]:
            f = field[i]
            rows.append((i, st, n, o) + (f if isinstance(f, tuple) else (-1, -1)))
            o += n + 1
        raw = words(lib, idx, 6 * nidx)
        got = [tuple(raw[6 * r:6 * r + 6]) for r in range(nidx)]
        assert got == rows, [(g, w) for g, w in zip(got, rows) if g != w][:3]
    finally:
        for b in (src, out, idx):
            if b:
                b.free()
    return info, want, rows


def lines_of(keys, rng, pads=(b"", b"x ", b"GET /a ", b"-- ")):
    """a buffer of lines `<pad>k=KEY <pad>`; every other buffer ends without a delimiter"""
    out = [pads[i % len(pads)] + b"k=" + k + b" " + pads[(i // 3) % len(pads)] for i, k in enumerate(keys)]
    return b"\n".join(out) + (b"\n" if rng.random() < 0.5 else b"")


def both_directions(p, data, **kw):
    res = []
    for desc in (False, True):
        res.append(run_text(p.sc, p.exp, data, desc=desc, src_off=3, dst_off=5, **kw))
    return res


# ------------------------------------------------------------------ 1 - 6. the order

def test_random_texts_three_chunks(gpu):
    """lengths 0 - 16 over {NUL, a, b, 0xff}: three chunks, many ties and many prefix pairs"""
    rng = random.Random(1)
    pool_ = [bytes(rng.choice(b"\0ab\xff") for _ in range(rng.randrange(17))) for _ in range(N // 3)]
    data = lines_of([rng.choice(pool_) for _ in range(N)], rng)
    with S.Pool() as pool:
        p = Program(pool, K)
        assert p.sc.engine == S.ENGINE_SCAN
        for info, _, _ in both_directions(p, data):
            assert (info.minlen, info.maxlen) == (0, 16) and info.passes == len(S.sort_text_plan(0, 16, False)) == 19
            assert p.sc.last_lines_device == 1


@pytest.mark.parametrize("first", [7, 14])
def test_texts_that_differ_only_behind_a_chunk(gpu, first):
    """a shared prefix of one or two whole chunks: a sort of chunk 0 alone (or of chunks 0 and 1) leaves them in line order"""
    rng = random.Random(first)
    tails = [bytes(rng.choice(b"abc\xff") for _ in range(rng.randrange(1, 7))) for _ in range(200)]
    data = lines_of([b"P" * first + rng.choice(tails) for _ in range(N)], rng)
    with S.Pool() as pool:
        p = Program(pool, K)
        for info, _, rows in both_directions(p, data):
            assert info.minlen == first + 1 and info.maxlen == first + 6


def test_the_prefix_chain(gpu):
    rng = random.Random(4)
    keys = [b"x" * k for k in range(21)] * 3
    rng.shuffle(keys)
    data = lines_of(keys, rng)
    with S.Pool() as pool:
        p = Program(pool, K)
        (_, _, up), (_, _, down) = both_directions(p, data)
        assert [r[5] for r in up] == sorted(r[5] for r in up) and [r[5] for r in down] == sorted((r[5] for r in down), reverse=True)


def test_the_cnt_tie_at_a_chunk_boundary_and_unsigned_bytes(gpu):
    rng = random.Random(5)
    ties = [b"aaaaaaa", b"aaaaaaa\0", b"aaaaaaab", b"a" * 14, b"a" * 14 + b"\0", b"a" * 14 + b"b", b"a", b"a\0", b"a\0\0", b"aa"]
    signed = [b"q\x7f", b"q\x80", b"q\xff", b"q\x7fz", b"\x7f", b"\x80", b"\xff", b"\xff" * 7, b"\xff" * 8]
    keys = (ties + signed) * 40
    rng.shuffle(keys)
    data = lines_of(keys, rng)
    with S.Pool() as pool:
        p = Program(pool, K)
        (_, out, rows), _ = both_directions(p, data)
        got = [data[r[4]:r[4] + r[5]] for r in rows]
        assert got == sorted(keys)
        first = [got.index(t) for t in (b"a", b"a\0", b"a\0\0", b"aa", b"aaaaaaa", b"aaaaaaa\0", b"aaaaaaab")]
        assert first == sorted(first)
        assert got.index(b"q\x7f") < got.index(b"q\x7fz") < got.index(b"q\x80") < got.index(b"q\xff") < got.index(b"\x7f")


# ------------------------------------------------------------------ 7 - 9. the cut, and what needs no pass

@pytest.mark.parametrize("max_bytes", [1, 3, 7, 8])
def test_max_bytes(gpu, max_bytes):
    """ties beyond the cut keep line order; minlen / maxlen are the cut lengths"""
    rng = random.Random(max_bytes)
    keys = [bytes(rng.choice(b"ab") for _ in range(rng.randrange(max(max_bytes - 1, 0), max_bytes + 6))) for _ in range(N)]
    data = lines_of(keys, rng)
    with S.Pool() as pool:
        p = Program(pool, K)
        for info, _, rows in both_directions(p, data, max_bytes=max_bytes):
            assert info.maxlen == max_bytes and info.minlen == max_bytes - 1
            assert max(r[5] for r in rows) > max_bytes, "the index has the full length"


@pytest.mark.parametrize("key", [b"the-same-text-19-by", b""])
def test_all_texts_equal(gpu, key):
    data = lines_of([key] * N, random.Random(8))
    with S.Pool() as pool:
        p = Program(pool, K)
        for info, out, rows in both_directions(p, data, shape=False):
            assert info.passes == len(S.sort_text_plan(len(key), len(key), False)) == len(key)
            assert [r[0] for r in rows] == list(range(N)) and out == (data if data.endswith(b"\n") else data + b"\n")


# ------------------------------------------------------------------ 10. descending, ALL, unset groups

def mixed_lines(rng, n):
    pool_ = [bytes(rng.choice(b"ab\0\xff") for _ in range(rng.randrange(10))) for _ in range(n // 4)]
    out = []
    for i in range(n):
        r = rng.random()
        out.append(b"nothing here %d" % i if r < 0.15 else b"x u= y" if r < 0.3 else b"p k=" + rng.choice(pool_) + b" q")
    return b"\n".join(out) + b"\n"


def test_descending_all_lines_and_unset_groups(gpu):
    rng = random.Random(10)
    data = mixed_lines(rng, N)
    with S.Pool() as pool:
        p = Program(pool, KU)
        for desc in (False, True):
            info, out, rows = run_text(p.sc, p.exp, data, 1, 0, desc, True, src_off=1, dst_off=9)
            assert info.nlines == info.nselected == N and 0 < info.nkeyed < N and info.minlen == 0
            assert sorted(out.split(b"\n")) == sorted(data.split(b"\n")), "a permutation of the input"
            tail = rows[info.nkeyed:]
            assert all(r[4:] == (-1, -1) and data[r[1]:r[1] + 7] == b"nothing" for r in tail) and [r[0] for r in tail] == sorted(r[0] for r in tail)
            unset = [r[0] for r in rows[:info.nkeyed] if r[4:] == (-1, -1)]
            empty = [r[0] for r in rows[:info.nkeyed] if r[5] == 0]
            assert unset and unset == sorted(unset)
            # the unset groups are empty texts: first ascending, last of the keyed descending
            block = rows[info.nkeyed - len(unset) - len(empty):info.nkeyed] if desc else rows[:len(unset) + len(empty)]
            assert sorted(r[0] for r in block) == sorted(unset + empty) == [r[0] for r in block]
            without, _, _ = run_text(p.sc, p.exp, data, 1, 0, desc, False, src_off=1, dst_off=9)
            assert without.nselected == info.nkeyed and without.passes == len(S.sort_text_plan(info.minlen, info.maxlen, False))
            # (lengths 0 - 9 leave the rest nothing to add: every digit of chunk 0 and both counts are in the plan already)
            assert info.passes == len(S.sort_text_plan(info.minlen, info.maxlen, True)) >= without.passes


# ------------------------------------------------------------------ 11. limits and capacities

def test_limits_truncation_and_the_sizing_call(gpu):
    rng = random.Random(11)
    data = mixed_lines(rng, 400)
    with S.Pool() as pool:
        p = Program(pool, KU)
        for desc, all_lines in ((False, False), (True, True)):
            full = run_text(p.sc, p.exp, data, 1, 0, desc, all_lines)
            n = full[0].nselected
            for limit in (1, 100, n, n + 1):
                info, out, rows = run_text(p.sc, p.exp, data, 1, 0, desc, all_lines, limit, shape=False)
                assert info.nselected == min(limit, n) and full[1].startswith(out) and rows == full[2][:len(rows)]
                assert (info.nkeyed, info.minlen, info.maxlen, info.passes) == (full[0].nkeyed, full[0].minlen, full[0].maxlen, full[0].passes)
            need = full[0].need_bytes
            sizing, nothing, _ = run_text(p.sc, p.exp, data, 1, 0, desc, all_lines, out_cap=0, null_out=True)
            assert sizing.need_bytes == need and sizing.nwritten == 0 and nothing == b""
            boundary = len(b"\n".join(full[1].split(b"\n")[:41])) + 1           # the end of row 41
            short, _, _ = run_text(p.sc, p.exp, data, 1, 0, desc, all_lines, out_cap=boundary - 1, dst_off=9)
            assert short.nwritten == 40 and short.need_bytes == need
            assert run_text(p.sc, p.exp, data, 1, 0, desc, all_lines, out_cap=boundary, dst_off=9)[0].nwritten == 41
            for icap in (0, 7):
                run_text(p.sc, p.exp, data, 1, 0, desc, all_lines, index_cap=icap, src_off=1)


def test_small_buffers(gpu):
    with S.Pool() as pool:
        p = Program(pool, KU)
        for desc in (False, True):
            assert run_text(p.sc, p.exp, b"", 1, 0, desc, True, shape=False)[0] == S.SortTextInfo(0, 0, 0, 0, 0, 0, 0, SIZE_MAX, 0)
            info, out, _ = run_text(p.sc, p.exp, b"k=one", 1, 0, desc, False, shape=False)
            assert info == S.SortTextInfo(1, 1, 1, 6, 1, 6, 3, 3, 3) and out == b"k=one\n"
            data = b"nothing\nat all\n\nhere"
            assert run_text(p.sc, p.exp, data, 1, 0, desc, False, shape=False)[0] == S.SortTextInfo(4, 0, 0, 0, 0, 0, 0, SIZE_MAX, 0)
            info, out, _ = run_text(p.sc, p.exp, data, 1, 0, desc, True, shape=False)
            assert info == S.SortTextInfo(4, 0, 4, len(data) + 1, 4, len(data) + 1, 0, SIZE_MAX, 0) and out == data + b"\n"
            data = b"k=b \nk=a \nzzz\nk=b \nk=a"          # the last line without a delimiter
            info, out, _ = run_text(p.sc, p.exp, data, 1, 0, desc, True, shape=False)
            assert out == (b"k=b \nk=b \nk=a \nk=a\nzzz\n" if desc else b"k=a \nk=a\nk=b \nk=b \nzzz\n")


# ------------------------------------------------------------------ 12. the NFA tier

def test_the_nfa_tier(gpu):
    rng = random.Random(12)
    names = [bytes(rng.choice(b"abc.") for _ in range(rng.randrange(13))) for _ in range(60)]
    lines = [b"GET t=%dms k=%s;" % (rng.randrange(1000), rng.choice(names)) if rng.random() < 0.85 else b"t=ms k=none" for _ in range(600)]
    data = b"\n".join(lines)
    with S.Pool() as pool:
        p = Program(pool, COUNTED, S.ENGINE_NFA)
        assert p.sc.engine == S.ENGINE_NFA
        for desc, all_lines in ((False, False), (True, True)):
            info, _, _ = run_text(p.sc, p.exp, data, 1, 0, desc, all_lines, src_off=3, dst_off=5)
            assert p.sc.last_lines_device == 1 and 0 < info.nkeyed < info.nlines


# ------------------------------------------------------------------ 13. a caller's stream, between other calls

def test_on_a_callers_gated_stream_between_other_calls(gpu):
    """the call on a non-blocking stream whose copy of the real input is held back by a gate: work issued on another stream
    would sort the decoy.  A numeric sort and a filter on the same scanner give the same before and after"""
    rng = random.Random(13)
    keys = [b"%02d" % rng.randrange(40) + bytes(rng.choice(b"ab") for _ in range(8)) for _ in range(N)]
    real = lines_of(keys, random.Random(1))
    rng.shuffle(keys)
    decoy = lines_of(keys, random.Random(1))
    assert len(real) == len(decoy) and real != decoy
    with S.Pool() as pool:
        p = Program(pool, [rb"k=(([0-9]*)[^ ]*)"])
        before = (run_sort(p.sc, p.exp, real, 2, True, True), run_filter(p.sc, p.exp, real, 0x0A, S.HIP_PIKE_FIRST))
        want = run_text(p.sc, p.exp, real, 1, 0, True, True)
        assert want != run_text(p.sc, p.exp, decoy, 1, 0, True, True)
        buf, src = S.DeviceBuffer.from_bytes(decoy), S.DeviceBuffer.from_bytes(real)
        try:
            with GatedStream() as gs:
                gs.produce(buf.ptr, src.ptr, len(real))
                assert gs.copy_pending(), "the gate does not hold the stream"
                got = run_text(p.sc, p.exp, real, 1, 0, True, True, stream=gs.handle, src_ptr=buf.ptr)
                assert not gs.timed_out
            assert got == want
        finally:
            buf.free()
            src.free()
        after = (run_sort(p.sc, p.exp, real, 2, True, True), run_filter(p.sc, p.exp, real, 0x0A, S.HIP_PIKE_FIRST))
        assert after == before


# ------------------------------------------------------------------ 14. composition

def test_two_calls_sort_by_two_columns(gpu):
    rng = random.Random(14)
    avals = [bytes(rng.choice(b"xyz") for _ in range(rng.randrange(1, 10))) for _ in range(12)]
    bvals = [bytes(rng.choice(b"pq\xff") for _ in range(rng.randrange(0, 9))) for _ in range(40)]
    rows = [(rng.choice(avals), rng.choice(bvals), rng.randrange(-50, 50)) for _ in range(N)]
    data = b"".join(b"a=%s b=%s n=%d\n" % r for r in rows)
    with S.Pool() as pool:
        p = Program(pool, AB)
        # by B, then by A on the output: (A, B, line)
        _, by_b, _ = run_text(p.sc, p.exp, data, 2)
        _, by_ab, _ = run_text(p.sc, p.exp, by_b, 1, shape=False)
        order = sorted(range(N), key=lambda i: (rows[i][0], rows[i][1], i))
        assert by_ab == b"".join(b"a=%s b=%s n=%d\n" % rows[i] for i in order)
        # a numeric sort, then the text sort on its output: (A, n, line)
        _, by_n, _ = run_sort(p.sc, p.exp, data, 3)
        _, by_an, _ = run_text(p.sc, p.exp, by_n, 1, shape=False)
        order = sorted(range(N), key=lambda i: (rows[i][0], rows[i][2], i))
        assert by_an == b"".join(b"a=%s b=%s n=%d\n" % rows[i] for i in order)
