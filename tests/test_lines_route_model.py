"""The partition of the line route (sre_hip_route_lines) on the CPU: tests/lines_route_sim.cpp runs count, scan and
scatter workgroup by workgroup and wave by wave with the rules the kernels compile (sregex_amd/csrc/sre_lines_route.h)
and counts every store to the compact table.  The table must be the stable bucket-major permutation of the routed lines;
fed through the extract's gather model (tests/lines_extract_sim.cpp, unchanged) it must write every output byte exactly
once.  A case is a list of lines and, per line, its bucket or None (dropped); the expected output is Python grouping."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32, _i64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
_p64, _p32, _p8 = ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_uint8)
_pi32 = ctypes.POINTER(ctypes.c_int32)
FILL = 0xA5
DELIM = 0x0A


def _build(name, source, headers):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, source)] + [os.path.join(csrc, h) for h in headers]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def rsim():
    L = _build("liblinesroutesim.so", "lines_route_sim.cpp", ["sre_lines_route.h", "sre_lines_gather.h"])
    L.lrsim_items.restype = _u32
    L.lrsim_flags.restype = _u64
    L.lrsim_start_mask.restype = _u64
    L.lrsim_key.restype = _u64
    L.lrsim_key.argtypes = [_i64, _u32, _pi32, _u64]
    L.lrsim_count.restype = _u32
    L.lrsim_count.argtypes = [_p64, _u64, _u32, _p64]
    L.lrsim_scan.restype = None
    L.lrsim_scan.argtypes = [_p64, _u64]
    L.lrsim_scatter.restype = _u64
    L.lrsim_scatter.argtypes = [_p64, _p64, _u64, _u32, _p64, _u64, _p64, _p64, _p64, _p32]
    L.lrsim_cut.restype = _u64
    L.lrsim_cut.argtypes = [_p64, _u64, _u64]
    L.lrsim_totals.restype = None
    L.lrsim_totals.argtypes = [_p64, _u64, _u32, _p64, _p64, _p64]
    L.lrsim_meta_bucket.restype = _u32
    L.lrsim_meta_bucket.argtypes = [_u64]
    L.lrsim_meta_line.restype = _u64
    L.lrsim_meta_line.argtypes = [_u64]
    return L


@pytest.fixture(scope="module")
def gsim():
    """the extract's gather model, as tests/test_lines_extract_model.py builds it (a library of its own here)"""
    L = _build("liblinesextractsim_route.so", "lines_extract_sim.cpp", ["sre_lines_gather.h"])
    L.lesim_gather.restype = _u64
    L.lesim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32,
                               _p64, _p64]
    return L


def make_lines(rng, n, longest=12):
    return [bytes(rng.choice(b"abcxyz .") for _ in range(rng.randrange(longest + 1))) for _ in range(n)]


def partition(rsim, lines, buckets, nb):
    """count / scan / scatter of the model; returns (first, nsel, cstart, coff, cmeta) after asserting the table"""
    n = len(lines)
    ends, pos = [], 0
    for ln in lines:
        ends.append(pos + len(ln))
        pos += len(ln) + 1
    # the keys through the select rule: regex r maps to bucket r, "no match" (rc -1) is dropped
    ident = (ctypes.c_int32 * (nb + 1))(*(list(range(nb)) + [-1]))
    keys = [rsim.lrsim_key(-1 if b is None else b, nb, ident, len(ln)) for ln, b in zip(lines, buckets)]
    for k, ln, b in zip(keys, lines, buckets):
        assert k == (0 if b is None else (b << 56) | (len(ln) + 1))
    a_key, a_ends = (_u64 * max(n, 1))(*keys), (_u64 * max(n, 1))(*ends)
    items = rsim.lrsim_items()
    nwg = (n + items - 1) // items
    first = (_u64 * (nb * nwg + 1))()
    turns = rsim.lrsim_count(a_key, n, nb, first)
    # the cost rule: a slot's loop takes one turn per distinct bucket present in it
    most = 0
    for s in range(0, n, 64):
        most = max(most, len({b for b in buckets[s:s + 64] if b is not None}))
    assert turns == most
    for w in range(nwg):
        for b in range(nb):
            assert first[b * nwg + w] == sum(1 for x in buckets[w * items:(w + 1) * items] if x == b)
    rsim.lrsim_scan(first, nb * nwg)
    nsel = first[nb * nwg]
    order = [i for b in range(nb) for i in range(n) if buckets[i] == b]      # stable, bucket-major
    assert nsel == len(order)
    cstart, cval, cmeta = (_u64 * max(nsel, 1))(), (_u64 * (nsel + 1))(), (_u64 * max(nsel, 1))()
    writes = (_u32 * max(nsel, 1))()
    bad = rsim.lrsim_scatter(a_key, a_ends, n, nb, first, nsel, cstart, cval, cmeta, writes)
    assert bad == 0
    assert list(writes)[:nsel] == [1] * nsel, "every entry of the compact table exactly once"
    flags, mask = rsim.lrsim_flags(), rsim.lrsim_start_mask()
    for r, i in enumerate(order):
        assert cstart[r] & ~mask == flags
        assert cstart[r] & mask == ends[i] - len(lines[i])
        assert cval[r] == len(lines[i]) + 1
        assert rsim.lrsim_meta_line(cmeta[r]) == i and rsim.lrsim_meta_bucket(cmeta[r]) == buckets[i]
    rsim.lrsim_scan(cval, nsel)
    return first, nsel, cstart, cval, cmeta, order


def run(rsim, gsim, lines, buckets, nb, src_off=0, dst_off=0, caps=(None,)):
    n = len(lines)
    d = bytes([DELIM])
    buf = b"".join(ln + d for ln in lines)
    first, nsel, cstart, coff, cmeta, order = partition(rsim, lines, buckets, nb)
    texts = [lines[i] + d for i in order]
    need = sum(len(t) for t in texts)
    assert coff[nsel] == need
    # the bucket totals of the finish pass
    for b in range(nb if nsel else 0):
        nl, by = _u64(), _u64()
        rsim.lrsim_totals(first, n, b, coff, ctypes.byref(nl), ctypes.byref(by))
        assert nl.value == sum(1 for x in buckets if x == b)
        assert by.value == sum(len(lines[i]) + 1 for i in range(n) if buckets[i] == b)
    src_len = (src_off + len(buf) + 15) // 16 * 16
    src = bytes([0xEE]) * src_off + buf + bytes([0xEE]) * (src_len - src_off - len(buf))
    for cap in caps:
        cap = need if cap is None else cap(need, [len(t) for t in texts])
        if cap < 0:
            continue
        want, k = b"", 0
        for t in texts:
            if len(want) + len(t) > cap:
                break
            want += t
            k += 1
        cut = rsim.lrsim_cut(coff, nsel, cap) if nsel else 0
        assert cut == k, (cap, cut, k)
        out_bytes = coff[cut] if nsel else 0
        assert out_bytes == len(want) <= cap
        if out_bytes == 0:
            continue        # (the call launches no gather)
        dst_len = (dst_off + out_bytes + 15) // 16 * 16
        dst = (ctypes.c_uint8 * dst_len)(*([FILL] * dst_len))
        reads, writes = (_u32 * max(src_len, 1))(), (_u32 * dst_len)()
        win, glo = _u64(), _u64()
        bad = gsim.lesim_gather(coff, cstart, nsel, out_bytes, src_off, dst_off, DELIM, DELIM, src, src_len, dst, dst_len, reads,
                                writes, ctypes.byref(win), ctypes.byref(glo))
        ctx = (n, nb, src_off, dst_off, cap, out_bytes)
        assert bad == 0, ("accesses outside the aligned extents", bad, ctx)
        got = bytes(dst)
        assert got[dst_off:dst_off + out_bytes] == want, ctx
        w = list(writes)
        assert w[dst_off:dst_off + out_bytes] == [1] * out_bytes, ("every output byte exactly once", ctx)
        assert not any(w[:dst_off]) and not any(w[dst_off + out_bytes:]), ("a write outside [out, out + out_bytes)", ctx)
        assert got[:dst_off] == bytes([FILL]) * dst_off and got[dst_off + out_bytes:] == bytes([FILL]) * (dst_len - dst_off - out_bytes)


# need, need - 1, one row, one row - 1, 0
CAPS = (None, lambda need, rows: need - 1, lambda need, rows: rows[0] if rows else 0,
        lambda need, rows: rows[0] - 1 if rows else 0, lambda need, rows: 0)

SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
NBUCKETS = (1, 2, 5, 64, 256)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nb", NBUCKETS)
def test_random_buckets(rsim, gsim, n, nb):
    rng = random.Random(n * 1000 + nb)
    lines = make_lines(rng, n)
    buckets = [rng.choice([None] + list(range(nb))) if rng.random() < 0.2 else rng.randrange(nb) for _ in range(n)]
    run(rsim, gsim, lines, buckets, nb, src_off=rng.randrange(16), dst_off=rng.randrange(16))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nb", NBUCKETS)
def test_one_bucket_takes_all(rsim, gsim, n, nb):
    rng = random.Random(n + nb)
    run(rsim, gsim, make_lines(rng, n), [nb - 1] * n, nb, src_off=3, dst_off=5)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nb", NBUCKETS)
def test_round_robin(rsim, gsim, n, nb):
    """with 64 buckets or more every full wave holds 64 distinct buckets"""
    rng = random.Random(n * 7 + nb)
    run(rsim, gsim, make_lines(rng, n), [i % nb for i in range(n)], nb, src_off=1, dst_off=15)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nb", NBUCKETS)
def test_all_dropped(rsim, gsim, n, nb):
    rng = random.Random(n)
    run(rsim, gsim, make_lines(rng, n), [None] * n, nb, caps=CAPS)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nb", (5, 64, 256))
def test_empty_bucket_in_the_middle(rsim, gsim, n, nb):
    rng = random.Random(n * 3 + nb)
    hole = nb // 2
    buckets = [rng.choice([b for b in range(nb) if b != hole]) for _ in range(n)]
    run(rsim, gsim, make_lines(rng, n), buckets, nb, src_off=7, dst_off=9)


@pytest.mark.parametrize("n", (1, 65, 1025, 2049))
@pytest.mark.parametrize("nb", (1, 5, 256))
def test_cuts(rsim, gsim, n, nb):
    rng = random.Random(n * 11 + nb)
    lines = make_lines(rng, n)
    lines[0] = b"first line"        # (one row - 1 is then a real capacity)
    buckets = [rng.randrange(nb) for _ in range(n)]
    buckets[0] = 0                  # (and that line is the first row of the output)
    run(rsim, gsim, lines, buckets, nb, src_off=2, dst_off=13, caps=CAPS)


def test_empty_lines_and_a_long_one(rsim, gsim):
    rng = random.Random(5)
    lines = make_lines(rng, 300, longest=3)
    lines[17] = bytes(rng.choice(b"abc") for _ in range(20000))
    for i in range(0, 300, 9):
        lines[i] = b""
    run(rsim, gsim, lines, [i % 3 if i % 5 else None for i in range(300)], 3, src_off=4, dst_off=11, caps=CAPS)


def test_error_rc_is_dropped(rsim):
    m = (ctypes.c_int32 * 3)(1, 0, 1)
    assert rsim.lrsim_key(0, 2, m, 4) == (1 << 56) | 5
    assert rsim.lrsim_key(1, 2, m, 0) == (0 << 56) | 1
    assert rsim.lrsim_key(-1, 2, m, 0) == (1 << 56) | 1       # no match: entry nreg
    assert rsim.lrsim_key(-2, 2, m, 9) == 0 and rsim.lrsim_key(2, 2, m, 9) == 0
