"""The line route (sre_hip_route_lines): every line of a device buffer goes to the bucket of the regex of its first
match; the output is one device buffer, bucket-major, line order inside a bucket, each line followed by one delimiter.

Expected output is pure Python: the split rule of line mode, the oracle's record of every line (its word 0 is the regex
id of the first match), the call's map, grouped and joined.  Output and index buffers have 64 guard bytes in front and
behind and are pre-filled with 0xA5; every check asserts that the guards and everything at or beyond what the call may
write still hold 0xA5.
"""
import ctypes
import random

import pytest

import sregex_amd as S
from test_gpu_lines import Expect, split_lines, upload_at
from test_gpu_lines_filter import Out, download

pytestmark = pytest.mark.gpu

FIRST = S.HIP_PIKE_FIRST
DOTTED = rb"\d{1,3}(\.\d{1,3}){3}"


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def setup(pool, pats, engine=S.ENGINE_AUTO, mode=FIRST):
    re = S.parse(pool, pats, multi=True)
    prog = S.compile(pool, re)
    return Expect(prog, re.ncaps, key=("route", tuple(pats))), S.Scanner(pool, prog, mode, engine), len(pats)


def expected(exp, data, delim, bucket_of, nbuckets, R):
    """[(line, start, len, bucket)] in output order, from the oracle's regex id of every line"""
    m = list(range(R)) + [-1] if bucket_of is None else list(bucket_of)
    assert len(m) == R + 1
    rows = []
    for i, (st, n) in enumerate(split_lines(data, delim)):
        rc = exp.record(data[st:st + n], FIRST)[0]
        assert rc == S.SRE_DECLINED or 0 <= rc < R
        b = m[R] if rc == S.SRE_DECLINED else m[rc]
        if b >= 0:
            rows.append((i, st, n, b))
    rows.sort(key=lambda r: r[3])           # stable: line order inside a bucket
    return rows


def run_route(sc, exp, data, R, bucket_of=None, nbuckets=None, delim=0x0A, src_off=0, dst_off=0, out_cap=None, index_cap=None,
              null_out=False):
    """one call, checked in full; returns (info, buckets, output bytes)"""
    lib = sc.lib
    d = bytes([delim])
    nb = nbuckets if nbuckets is not None else (R if bucket_of is None else max(bucket_of) + 1)
    rows = expected(exp, data, delim, bucket_of, nb, R)
    need = sum(n + 1 for _, _, n, _ in rows)
    cap = need + 37 if out_cap is None else out_cap
    nwritten, out_bytes = 0, 0
    for _, _, n, _ in rows:
        if out_bytes + n + 1 > cap:
            break
        out_bytes += n + 1
        nwritten += 1
    want = b"".join(data[st:st + n] + d for _, st, n, _ in rows[:nwritten])
    want_buckets, at = [], 0
    for b in range(nb):
        mine = [r for r in rows if r[3] == b]
        by = sum(r[2] + 1 for r in mine)
        want_buckets.append(S.RouteBucket(len(mine), at, by))
        at += by
    icap = len(rows) + 3 if index_cap is None else index_cap
    src = upload_at(data, src_off)
    out = Out(lib, cap, dst_off)
    idx = Out(lib, icap * 40, 0)
    try:
        info, buckets = sc.route_lines(src.ptr + src_off, len(data), None if null_out else out.ptr, cap, bucket_of, nb, delim,
                                       idx.ptr if icap else None, icap)
        assert info == S.FilterInfo(len(split_lines(data, delim)), len(rows), need, nwritten, out_bytes), (info, len(rows), need)
        assert buckets == want_buckets, [(b, g, w) for b, (g, w) in enumerate(zip(buckets, want_buckets)) if g != w][:3]
        out.check(want)
        nrows = min(icap, nwritten)
        wrows, o = [], 0
        for i, st, n, b in rows[:nrows]:
            wrows.append((i, st, n, o, b))
            o += n + 1
        raw = (ctypes.c_int64 * (5 * nrows)).from_buffer_copy(download(lib, idx.ptr, 40 * nrows)) if nrows else []
        got = [tuple(raw[5 * r:5 * r + 5]) for r in range(nrows)]
        assert got == wrows, [(g, w) for g, w in zip(got, wrows) if g != w][:3]
        idx.check(download(lib, idx.ptr, 40 * nrows))       # nothing behind the rows, nothing around the index
    finally:
        src.free()
        out.free()
        idx.free()
    return info, buckets, want


# ------------------------------------------------------------------ 1. the split

def test_split_edges(gpu):
    with S.Pool() as pool:
        exp, sc, R = setup(pool, [rb"a", rb"^$|b"])         # the second matches the empty line
        for delim in (0x0A, 0, 255):
            d = bytes([delim])
            for data in [b"", d, b"a" + d + d + b"b", b"a", d * 5, d * 40 + b"a", b"a" + d, b"b" + d + b"a" + d + d]:
                for m in (None, [0, 1, 2], [1, 1, 0], [-1, 0, -1]):
                    info, buckets, _ = run_route(sc, exp, data, R, m, delim=delim)
                if data == b"":
                    assert info == S.FilterInfo(0, 0, 0, 0, 0) and buckets == [S.RouteBucket(0, 0, 0)]
        info, buckets, want = run_route(sc, exp, b"\n" * 300, R)
        assert info.nselected == 300 and want == b"\n" * 300 and buckets[1].nlines == 300


# ------------------------------------------------------------------ 2. priority

def test_priority_is_the_oracles(gpu):
    pats = [rb"ab", rb"a", rb"b+"]
    lines = [b"ab", b"a", b"b", b"bab", b"xab", b"ba", b"bba", b"aab", b"xxbbb a", b"", b"zzz", b"abab", b"b a ab", b"a b ab"]
    with S.Pool() as pool:
        exp, sc, R = setup(pool, pats)
        data = b"\n".join(lines)
        ids = [exp.record(ln, FIRST)[0] for ln in lines]
        # leftmost first, then the lowest regex: "bab" belongs to b+ although ab and a match it too, "aab" to a
        assert ids[lines.index(b"bab")] == 2 and ids[lines.index(b"aab")] == 1 and ids[lines.index(b"ab")] == 0
        assert {0, 1, 2, S.SRE_DECLINED} == set(ids)
        info, buckets, _ = run_route(sc, exp, data, R, [0, 1, 2, 3], src_off=3, dst_off=9)
        assert [b.nlines for b in buckets] == [ids.count(0), ids.count(1), ids.count(2), ids.count(S.SRE_DECLINED)]
        assert sc.engine == S.ENGINE_SCAN and sc.last_lines_device == 1


# ------------------------------------------------------------------ 3. workgroup and wave boundaries

FIVE = [rb"alpha", rb"bravo", rb"charlie", rb"delta", rb"echo"]
WORDS = [b"alpha", b"bravo", b"charlie", b"delta", b"echo", b"none"]


def keyed_lines(n, pattern, seed):
    """n short lines; line i holds the word of rule pattern(i) (5: no rule's)"""
    rng = random.Random(seed)
    pads = [b"", b" ", b"x ", b"-- "]
    pick = {"random": lambda i: rng.randrange(6), "round-robin": lambda i: i % 6, "one": lambda i: 3}[pattern]
    return b"\n".join(pads[i % 4] + WORDS[pick(i)] + pads[(i // 4) % 4] for i in range(n)) + (b"\n" if n % 2 else b"")


ALIGN = [(0, 0), (1, 15), (7, 7), (15, 1)]


@pytest.mark.parametrize("n", [1023, 1024, 1025, 3000])
def test_workgroup_and_wave_boundaries(gpu, n):
    with S.Pool() as pool:
        exp, sc, R = setup(pool, FIVE)
        k = 0
        for pattern in ("random", "round-robin", "one"):
            data = keyed_lines(n, pattern, n)
            for m in ([0, 1, 2, 3, 4, 5], [-1] * 6):
                for src_off, dst_off in (ALIGN if m[0] == 0 else ALIGN[1:2]):
                    info, buckets, _ = run_route(sc, exp, data, R, m, 6, src_off=src_off, dst_off=dst_off)
                    assert info.nlines == n and info.nselected == (n if m[0] == 0 else 0)
                    if m[0] == 0:
                        assert [x.nlines for x in buckets] == [0, 0, 0, n, 0, 0] if pattern == "one" else all(x.nlines for x in buckets)
                    k += 1
        assert sc.last_lines_device == 1 and k == 15


# ------------------------------------------------------------------ 4. the forms of the map

def test_map_forms(gpu):
    data = keyed_lines(700, "random", 5)
    with S.Pool() as pool:
        exp, sc, R = setup(pool, FIVE)
        info, buckets, _ = run_route(sc, exp, data, R, None, src_off=5, dst_off=3)          # identity, the rest dropped
        assert len(buckets) == 5 and 0 < info.nselected < info.nlines and all(b.nlines for b in buckets)
        run_route(sc, exp, data, R, [1, 0, 1, 0, 1, 0], src_off=1)                           # many to one
        run_route(sc, exp, data, R, [2, -1, 0, -1, 1, -1], dst_off=11)                       # dropped rules
        run_route(sc, exp, data, R, [0, 1, 3, 4, 5, 2], src_off=9, dst_off=2)                # the rest in the middle
        run_route(sc, exp, data, R, [4, -1, -1, -1, -1, -1], 7)                               # empty buckets around one
        run_route(sc, exp, data, R, None)                                                    # the first map again


@pytest.mark.parametrize("invert", [False, True])
def test_grep_maps_reproduce_filter_lines(gpu, invert):
    data = keyed_lines(1500, "random", 6)
    with S.Pool() as pool:
        exp, sc, R = setup(pool, FIVE)
        m = [-1] * R + [0] if invert else [0] * R + [-1]
        info, buckets, routed = run_route(sc, exp, data, R, m, 1, src_off=3, dst_off=6)
        src = upload_at(data, 3)
        cap = len(data) + 8
        out, idx, ridx = Out(gpu, cap, 6), Out(gpu, 32 * info.nselected, 0), Out(gpu, 40 * info.nselected, 0)
        try:
            finfo = sc.filter_lines(src.ptr + 3, len(data), out.ptr, cap, invert=invert, index_ptr=idx.ptr, index_cap=info.nselected)
            assert finfo == info and 0 < info.nselected < info.nlines
            out.check(routed)
            rinfo, _ = sc.route_lines(src.ptr + 3, len(data), out.ptr, cap, m, 1, index_ptr=ridx.ptr, index_cap=info.nselected)
            assert rinfo == info
            out.check(routed)
            f = (ctypes.c_int64 * (4 * info.nselected)).from_buffer_copy(download(gpu, idx.ptr, 32 * info.nselected))
            r = (ctypes.c_int64 * (5 * info.nselected)).from_buffer_copy(download(gpu, ridx.ptr, 40 * info.nselected))
            assert [tuple(f[4 * k:4 * k + 4]) for k in range(info.nselected)] == [tuple(r[5 * k:5 * k + 4]) for k in range(info.nselected)]
        finally:
            for b in (src, out, idx, ridx):
                b.free()


# ------------------------------------------------------------------ 5. many buckets

def test_64_rules_plus_rest(gpu):
    rng = random.Random(64)
    pats = [b"k%02d" % r for r in range(64)]
    lines = []
    for i in range(4096):
        r = rng.randrange(66)
        lines.append(b"" if r == 65 else b"rest" if r == 64 else (b"", b"- ")[i % 2] + pats[r])
    lines[1234] = b"y" * 17000 + b" k07 k03"
    assert lines.count(b"") > 20
    data = b"\n".join(lines)
    with S.Pool() as pool:
        exp, sc, R = setup(pool, pats)
        # (AUTO gives this program to the NFA tier, first match on the device; the tests above run on the table-driven scanner)
        assert gpu.sre_hip_scanner_engine(sc.h) == S.ENGINE_NFA
        info, buckets, _ = run_route(sc, exp, data, R, list(range(65)), src_off=7, dst_off=13)
        assert sc.last_lines_device == 1
        assert info.nselected == 4096 and all(b.nlines for b in buckets)
        assert buckets[7].bytes > 17000 and buckets[64].nlines == lines.count(b"") + lines.count(b"rest")
        # every second rule dropped, the others folded onto 256 buckets' highest numbers
        m = [255 - r // 2 if r % 2 == 0 else -1 for r in range(64)] + [0]
        info, buckets, _ = run_route(sc, exp, data, R, m, 256, src_off=1, dst_off=2)
        assert buckets[255].nlines and buckets[0].nlines and not buckets[100].nlines


# ------------------------------------------------------------------ 6. truncation

def test_truncation(gpu):
    data = keyed_lines(200, "random", 8)
    with S.Pool() as pool:
        exp, sc, R = setup(pool, FIVE)
        m = [3, 0, 1, 2, -1, 1]
        rows = expected(exp, data, 0x0A, m, 4, R)
        need, first = sum(n + 1 for _, _, n, _ in rows), rows[0][2] + 1
        full, totals, _ = run_route(sc, exp, data, R, m, 4)
        assert full.nwritten == len(rows) > 50 and first > 1
        for dst_off in (0, 5):
            for cap, nwritten in [(need, len(rows)), (need - 1, len(rows) - 1), (first, 1), (first - 1, 0), (0, 0)]:
                info, buckets, _ = run_route(sc, exp, data, R, m, 4, src_off=1, dst_off=dst_off, out_cap=cap)
                assert info.nwritten == nwritten and info.need_bytes == need and info.nselected == len(rows)
                assert buckets == totals                    # the bucket totals do not depend on the cap
        info, buckets, _ = run_route(sc, exp, data, R, m, 4, out_cap=0, null_out=True, index_cap=0)      # a sizing call
        assert info == S.FilterInfo(200, len(rows), need, 0, 0) and buckets == totals
        for icap in (0, 1, len(rows) + 3):
            info, _, _ = run_route(sc, exp, data, R, m, 4, index_cap=icap)
            assert info.nwritten == len(rows)
        info, _, _ = run_route(sc, exp, data, R, m, 4, out_cap=need // 2, index_cap=None)
        assert 3 < info.nwritten < len(rows)


# ------------------------------------------------------------------ 7. batch cuts

def test_batch_cuts(gpu, monkeypatch):
    data = keyed_lines(3000, "random", 9)
    with S.Pool() as pool:
        exp, sc, R = setup(pool, FIVE)
        _, _, one = run_route(sc, exp, data, R, [0, 1, 2, 3, 4, 5], src_off=2, dst_off=9)
        assert sc.last_line_batches == 1
        monkeypatch.setenv("SRE_HIP_LINES_BATCH", "700")
        _, _, many = run_route(sc, exp, data, R, [0, 1, 2, 3, 4, 5], src_off=2, dst_off=9)
        assert sc.last_line_batches == 5 and many == one
        run_route(sc, exp, data, R, [2, -1, 0, -1, 1, -1])
        assert sc.last_line_batches == 5


# ------------------------------------------------------------------ 8. the other routes

def dotted_lines(n, seed):
    rng = random.Random(seed)
    words = [b"10.0.0.255", b"host 1.22.3.4 up", b"error: disk", b"an error 9.9.9.9", b"1.2.3", b"", b"nothing", b"7.7.7.7 error"]
    return b"\n".join(rng.choice(words) for _ in range(n))


@pytest.mark.parametrize("engine,host", [(S.ENGINE_NFA, 0), (S.ENGINE_NFA, 1), (S.ENGINE_VM, 0)], ids=["nfa", "nfa-host", "vm"])
def test_other_routes(gpu, monkeypatch, engine, host):
    data = dotted_lines(300, 10)
    with S.Pool() as pool:
        exp, sc, R = setup(pool, [DOTTED, rb"error"], engine)
        assert sc.engine == engine
        if host:
            monkeypatch.setenv("SRE_HIP_LINES_NFA_HOST", "1")
        device = 1 if engine == S.ENGINE_NFA and not host else 0
        for m in (None, [0, 1, 2], [1, -1, 0]):
            info, buckets, _ = run_route(sc, exp, data, R, m, src_off=3, dst_off=5)
            assert sc.last_lines_device == device
            assert info.nlines == 300 and all(b.nlines for b in buckets)


# ------------------------------------------------------------------ 9. refusals

def test_refusals(gpu):
    data = keyed_lines(50, "random", 11)
    with S.Pool() as pool:
        re = S.parse(pool, FIVE, multi=True)
        prog = S.compile(pool, re)
        first = S.Scanner(pool, prog, FIRST)
        src = upload_at(data, 0)
        out = Out(gpu, 4096, 0)
        info = (ctypes.c_size_t * 5)(*([77] * 5))
        bk = (ctypes.c_size_t * (3 * 257))(*([77] * (3 * 257)))

        def call(sc, m, nb, d_out=None, cap=4096):
            arr = (ctypes.c_int * len(m))(*m) if m is not None else None
            rc = gpu.sre_hip_route_lines(sc.h, src.ptr, len(data), 0x0A, arr, nb, out.ptr if d_out is None else d_out, cap, None, 0,
                                         info, bk, None)
            assert list(info) == [77] * 5 and set(bk) == {77}, "a refused call wrote its results"
            return rc

        try:
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_COUNT):
                assert call(S.Scanner(pool, prog, mode), [0, 1, 2, 3, 4, 5], 6) == -1
            assert call(first, [0] * 6, 0) == -1
            assert call(first, [0] * 6, 257) == -1
            assert call(first, [0, 1, 2, 3, 4, 6], 6) == -1            # a value >= nbuckets
            assert call(first, [0, 1, 2, 3, 4, -2], 6) == -1
            assert call(first, None, 4) == -1 and call(first, None, 6) == -1       # NULL map: nbuckets must be R
            assert call(first, [0] * 6, 1, d_out=src.ptr + 10, cap=20) == -1     # the output inside the source
            assert call(first, [0] * 6, 1, d_out=src.ptr - 8, cap=9) == -1       # ... and over its first byte
            out.check(b"")
            assert download(gpu, src.ptr, len(data)) == data
            with pytest.raises(RuntimeError):
                first.route_lines(src.ptr, len(data), out.ptr, 4096, [0, 1, 2, 3, 4, 9], 6)
            # and the same scanner still routes
            rinfo, _ = first.route_lines(src.ptr, len(data), out.ptr, 4096, [0] * 6, 1)
            assert rinfo.nselected == rinfo.nwritten == 50
        finally:
            src.free()
            out.free()


# ------------------------------------------------------------------ 10. idempotence

def test_routing_a_buckets_slice_again_keeps_it_whole(gpu):
    data = keyed_lines(900, "random", 12)
    with S.Pool() as pool:
        exp, sc, R = setup(pool, FIVE)
        m = [0, 1, 2, 3, 4, 5]
        info, buckets, once = run_route(sc, exp, data, R, m, 6, src_off=7, dst_off=1)
        assert sum(b.bytes for b in buckets) == len(once) == info.need_bytes
        for b, bk in enumerate(buckets):
            piece = once[bk.offset:bk.offset + bk.bytes]
            assert bk.nlines and piece.endswith(b"\n")
            info2, buckets2, twice = run_route(sc, exp, piece, R, m, 6, src_off=1, dst_off=7)
            assert twice == piece and info2.nlines == info2.nselected == bk.nlines
            assert buckets2 == [S.RouteBucket(bk.nlines, 0, bk.bytes) if x == b else S.RouteBucket(0, 0 if x < b else bk.bytes, 0)
                                for x in range(6)]
