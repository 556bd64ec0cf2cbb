"""The line sort by text (sre_hip_sort_lines_text) on the CPU: tests/lines_sort_text_sim.cpp runs the values pass, the keys of
every chunk, the pass that makes the items and every later digit pass with the rules the kernels compile
(sregex_amd/csrc/sre_lines_sort_text.h) and counts every store and every byte read outside the buffer.  The chunk keys compare
as Python's bytes do; the descending and the rest keys keep their places; the plan holds every (chunk, digit) at which two keys
can differ and has the stated lengths; the whole model equals sorted() with stable ties; and fed through the extract's gather
model (tests/lines_extract_sim.cpp, unchanged) every output byte is written once.  A case is a list of (text of the line,
field) with field = (offset, length) of the sort group, "unset", or None for a line without a match."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32, _i64, _u8, _i8 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint8, ctypes.c_int8
_p64, _p32, _p8, _pi64, _pi8 = (ctypes.POINTER(t) for t in (_u64, _u32, _u8, _i64, _i8))
_int = ctypes.c_int
FILL = 0xA5
DELIM = 0x0A
ALPHABET = (0x00, 0x01, ord("a"), 0x7F, 0x80, 0xFF)
SIZE_MAX = (1 << 64) - 1


def _build(name, source, headers):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, source)] + [os.path.join(csrc, h) for h in headers] + [os.path.join(HERE, "lines_sort_sim.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def tsim():
    L = _build("liblinessorttextsim.so", "lines_sort_text_sim.cpp",
               ["sre_lines_sort_text.h", "sre_lines_sort.h", "sre_lines_sums.h", "sre_lines_route_key.h", "sre_lines_route.h",
                "sre_lines_gather.h"])
    for name in ("lstsim_kmax", "lstsim_rest", "lsosim_flags", "lsosim_start_mask", "lsosim_unset", "lsosim_dropped"):
        getattr(L, name).restype = _u64
    L.lstsim_chunk.restype = _u32
    L.lstsim_cut.restype = _u64
    L.lstsim_cut.argtypes = [_u64, _u64]
    L.lstsim_dir.restype = _u64
    L.lstsim_dir.argtypes = [_u64, _int]
    L.lstsim_rest_key.restype = _u64
    L.lstsim_rest_key.argtypes = [_u64, _int]
    L.lstsim_chunk_key.restype = _u64
    L.lstsim_chunk_key.argtypes = [ctypes.c_char_p, _u64, _u64, _u64, _p64]
    L.lstsim_plan.restype = _u64
    L.lstsim_plan.argtypes = [_u64, _u64, _int, _p64, _u64]
    L.lstsim_index_row.restype = _u64
    L.lstsim_index_row.argtypes = [ctypes.c_char_p, _u64, _p64, _p64, _u64, _p64, _p64, _u64, _pi64]
    L.lstsim_sort.restype = _u64
    L.lstsim_sort.argtypes = [ctypes.c_char_p, _u64, _p64, _p64, _u64, _u64, _int, _int, _p32, _p64]
    L.lsosim_limited.restype = _u64
    L.lsosim_limited.argtypes = [_u64, _u64]
    L.lsosim_table.restype = None
    L.lsosim_table.argtypes = [_p32, _p64, _u64, _u64, _p64, _p64, _p32]
    L.lsosim_scan.restype = None
    L.lsosim_scan.argtypes = [_p64, _u64]
    L.lsosim_result.restype = None
    L.lsosim_result.argtypes = [_p64, _u64, _u64, _p64]
    return L


@pytest.fixture(scope="module")
def gsim():
    """the extract's gather model, as tests/test_lines_extract_model.py builds it (a library of its own here)"""
    L = _build("liblinesextractsim_sort_text.so", "lines_extract_sim.cpp", ["sre_lines_gather.h"])
    L.lesim_gather.restype = _u64
    L.lesim_gather.argtypes = [_p64, _p64, _u64, _u64, _u32, _u32, _u32, _u32, ctypes.c_char_p, _u64, _p8, _u64, _p32, _p32,
                               _p64, _p64]
    return L


def chunk_keys(tsim, t, nchunks, desc=False):
    """the keys of chunks 0 .. nchunks - 1 of the text t, every byte read inside it"""
    bad = _u64()
    keys = [tsim.lstsim_dir(tsim.lstsim_chunk_key(t, len(t), len(t), c, ctypes.byref(bad)), int(desc)) for c in range(nchunks)]
    assert bad.value == 0
    return keys


def py_chunk_key(t, c):
    """the rule spelled out: seven bytes big-endian, 0 past the end, and the count in the low byte"""
    part = t[7 * c:7 * c + 7]
    return int.from_bytes(part.ljust(7, b"\0"), "big") << 8 | len(part)


def plan(tsim, minlen, maxlen, rest):
    n = tsim.lstsim_plan(minlen, maxlen, int(rest), None, 0)
    pairs = (_u64 * (2 * max(n, 1)))()
    assert tsim.lstsim_plan(minlen, maxlen, int(rest), pairs, n) == n
    return [(pairs[2 * i], pairs[2 * i + 1]) for i in range(n)]


def texts_of(lengths, per_length, rng):
    out = []
    for ln in lengths:
        total = len(ALPHABET) ** ln
        if total <= per_length:
            out += [bytes(t) for t in itertools.product(ALPHABET, repeat=ln)]
        else:
            out += [bytes(rng.choice(ALPHABET) for _ in range(ln)) for _ in range(per_length)]
    return out


def test_constants(tsim):
    assert tsim.lstsim_chunk() == 7 and tsim.lstsim_kmax() == 0xFFFFFFFFFFFFFF07 and tsim.lstsim_rest() == 0xFFFFFFFFFFFFFF08
    assert tsim.lstsim_rest() != tsim.lsosim_dropped() == SIZE_MAX
    assert [tsim.lstsim_cut(ln, m) for ln, m in ((5, 0), (5, 9), (5, 5), (5, 4), (0, 3))] == [5, 5, 5, 4, 0]


def test_chunk_keys_compare_as_bytes_do(tsim):
    """all pairs of texts of length 0 - 15 over the alphabet, the longer lengths sampled: comparing the chunk keys from chunk 0
    is Python's comparison of bytes (unsigned, a proper prefix first), and the descending keys mirror it"""
    rng = random.Random(7)
    texts = texts_of(range(0, 3), 40, rng) + texts_of(range(3, 16), 12, rng)
    # prefix pairs and NUL tails at the chunk boundaries
    for k in (6, 7, 8, 13, 14, 15):
        base = bytes(rng.choice(ALPHABET) for _ in range(k))
        texts += [base, base + b"\0", base + b"\0\0", base + b"\x01", base[:-1]]
    texts += [b"a", b"a\0", b"a\0\0", b"aa"]
    asc = [chunk_keys(tsim, t, 3) for t in texts]
    dsc = [chunk_keys(tsim, t, 3, desc=True) for t in texts]
    for t, k in zip(texts, asc):
        assert k == [py_chunk_key(t, c) for c in range(3)], t
    kmax = tsim.lstsim_kmax()
    for a, d in zip(asc, dsc):
        assert d == [kmax - k for k in a] and all(x <= kmax for x in a)
    for i, j in itertools.product(range(len(texts)), repeat=2):
        a, b = texts[i], texts[j]
        assert (asc[i] < asc[j]) == (a < b) and (asc[i] == asc[j]) == (a == b), (a, b)
        assert (dsc[i] < dsc[j]) == (a > b), (a, b)
    order = sorted(texts)
    assert order.index(b"a") < order.index(b"a\0") < order.index(b"a\0\0") < order.index(b"aa")


def test_rest_keys(tsim):
    """a line without a match under ALL: above every text's key in chunk 0, in both directions, the empty chunk's key elsewhere,
    and never the dropped key"""
    kmax, rest = tsim.lstsim_kmax(), tsim.lstsim_rest()
    worst = b"\xff" * 7
    for desc in (0, 1):
        assert tsim.lstsim_rest_key(0, desc) == rest == kmax + 1
        for t in (b"", worst, b"\xff" * 20, b"\0"):
            assert chunk_keys(tsim, t, 1, desc)[0] < rest
        for c in (1, 2, 9):
            assert tsim.lstsim_rest_key(c, desc) == chunk_keys(tsim, b"", c + 1, desc)[c] == (kmax if desc else 0)


@pytest.mark.parametrize("rest", [False, True])
def test_plan_holds_every_digit_at_which_two_keys_can_differ(tsim, rest):
    """brute force: for minlen / maxlen / rest, the keys of texts of every length in between over bytes {0, 0xff} (enough to
    set or clear every bit of every byte digit), both directions, with the rest's keys: every differing (chunk, digit) is in
    the plan, and the plan runs last chunk first with ascending digits"""
    rng = random.Random(11)
    for minlen, maxlen in [(a, b) for a in range(0, 17) for b in range(a, 17)]:
        got = plan(tsim, minlen, maxlen, rest)
        assert got == sorted(got, key=lambda cd: (-cd[0], cd[1])) and len(set(got)) == len(got)
        nch = maxlen // 7 + 2
        assert all(c < nch for c, _ in got)
        texts = []
        for ln in {minlen, maxlen, (minlen + maxlen) // 2, min(minlen + 1, maxlen), max(maxlen - 1, minlen)}:
            texts += [b"\0" * ln, b"\xff" * ln] + [bytes(rng.choice((0, 0xFF)) for _ in range(ln)) for _ in range(3)]
        union = set()
        for desc in (False, True):
            keys = [chunk_keys(tsim, t, nch, desc) for t in texts]
            if rest:
                keys.append([tsim.lstsim_rest_key(c, int(desc)) for c in range(nch)])
            differ = set()
            for a, b in itertools.combinations(keys, 2):
                for c in range(nch):
                    x = a[c] ^ b[c]
                    differ |= {(c, d) for d in range(8) if (x >> (8 * d)) & 0xFF}
            assert differ <= set(got), (minlen, maxlen, rest, desc, sorted(differ - set(got)))
            union |= differ
        # ... and nothing else: with both extreme lengths, all zeros and all ones present, the plan (which does not know the
        # direction) is exactly the digits that differ in one direction or the other
        assert union == set(got), (minlen, maxlen, rest, sorted(set(got) - union))


def test_plan_lengths(tsim):
    for ln in (0, 1, 6, 7, 8, 14, 15):
        assert len(plan(tsim, ln, ln, False)) == ln, ln
    assert plan(tsim, 0, 0, False) == [] and plan(tsim, SIZE_MAX, 0, True) == [] and plan(tsim, SIZE_MAX, 0, False) == []
    assert plan(tsim, 0, 0, True) == [(0, d) for d in range(8)]
    assert plan(tsim, 8, 8, False) == [(1, 7)] + [(0, d) for d in range(1, 8)]
    assert plan(tsim, 3, 9, False) == [(1, 0), (1, 6), (1, 7)] + [(0, d) for d in range(8)]
    # a chunk wholly below minlen has no count digit, the last chunk no byte digits past maxlen
    assert plan(tsim, 7, 9, False) == [(1, 0), (1, 6), (1, 7)] + [(0, d) for d in range(1, 8)]
    assert len(plan(tsim, 40, 40, False)) == 40 and len(plan(tsim, 0, 40, False)) == 40 + 6
    assert len(plan(tsim, 1000, 1000, False)) == 1000      # linear in maxlen


def line_of(rng, key, pad=None):
    """a line `<pad>k=<key> <pad>` and its field"""
    pad = bytes(rng.choice(b"abcxyz.") for _ in range(rng.randrange(6))) if pad is None else pad
    return pad + b"k=" + key + b" " + pad, (len(pad) + 2, len(key))


def random_key(rng, maxlen, alphabet=(0x00, ord("a"), ord("b"), 0xFF)):
    return bytes(rng.choice(alphabet) for _ in range(rng.randrange(maxlen + 1)))


def make_case(rng, n, maxlen, holes):
    case = []
    for _ in range(n):
        r = rng.random()
        if holes and r < 0.15:
            case.append((b"no key here", None))
        elif holes and r < 0.25:
            case.append((b"k", "unset"))
        else:
            case.append(line_of(rng, random_key(rng, maxlen)))
    return case


def layout(case):
    buf = b"".join(t + bytes([DELIM]) for t, _ in case)
    ends, pos = [], 0
    for t, _ in case:
        ends.append(pos + len(t))
        pos += len(t) + 1
    return buf, ends


def table_of(tsim, case):
    n = len(case)
    buf, ends = layout(case)
    flags, unset = tsim.lsosim_flags(), tsim.lsosim_unset()
    vval, vstart = (_u64 * max(n, 1))(), (_u64 * max(n, 1))()
    for i, (t, f) in enumerate(case):
        st = ends[i] - len(t)
        if f is None:
            vval[i], vstart[i] = 0, st | unset | flags
        elif f == "unset":
            vval[i], vstart[i] = 1, st | unset | flags
        else:
            vval[i], vstart[i] = f[1] + 1, (st + f[0]) | flags
    return buf, ends, vval, vstart


def field_text(case, i):
    t, f = case[i]
    return None if f is None else b"" if f == "unset" else t[f[0]:f[0] + f[1]]


def expected(case, max_bytes, desc, all_lines):
    keyed = [i for i in range(len(case)) if case[i][1] is not None]
    cut = {i: field_text(case, i)[:max_bytes] if max_bytes else field_text(case, i) for i in keyed}
    order = sorted(keyed, key=lambda i: cut[i], reverse=desc)        # (stable in both directions)
    rest = [i for i in range(len(case)) if case[i][1] is None] if all_lines else []
    lens = [len(cut[i]) for i in keyed]
    return order + rest, len(keyed), (min(lens) if lens else SIZE_MAX), (max(lens) if lens else 0), bool(rest)


def model_sort(tsim, case, max_bytes=0, desc=False, all_lines=False):
    """the whole model against sorted(); returns the order"""
    n = len(case)
    buf, ends, vval, vstart = table_of(tsim, case)
    out, info = (_u32 * max(n, 1))(), (_u64 * 5)()
    bad = tsim.lstsim_sort(buf, len(buf), vval, vstart, n, max_bytes, int(desc), int(all_lines), out, info)
    assert bad == 0, ("a read outside the buffer, a store outside an array or a word not written once", bad)
    want, nkeyed, minlen, maxlen, rest = expected(case, max_bytes, desc, all_lines)
    assert list(info)[:4] == [nkeyed, len(want), minlen, maxlen]
    assert info[4] == len(plan(tsim, minlen, maxlen, rest))
    assert list(out)[:len(want)] == want, (n, max_bytes, desc, all_lines)
    return want


@pytest.mark.parametrize("n", [0, 1, 2, 63, 65, 1023, 1025, 2500, 5000])
def test_whole_model_against_sorted(tsim, n):
    rng = random.Random(n)
    case = make_case(rng, n, 16, holes=True)
    combos = [(0, False, False), (0, True, True), (3, True, False), (8, False, True)] if n > 1100 else \
        [(m, d, a) for m in (0, 1, 7, 8) for d in (False, True) for a in (False, True)]
    for max_bytes, desc, all_lines in combos:
        model_sort(tsim, case, max_bytes, desc, all_lines)


def test_model_edges(tsim):
    rng = random.Random(3)
    # all texts equal, all empty, all unset, nothing keyed: line order, and no pass that is not needed
    for key in (b"same-key-of-19-bytes", b""):
        case = [line_of(rng, key) for _ in range(300)]
        for desc in (False, True):
            assert model_sort(tsim, case, 0, desc, False) == list(range(300))
    case = [(b"k", "unset")] * 70 + [(b"zzz", None)] * 5
    assert model_sort(tsim, case, 0, True, True) == list(range(75))
    case = [(b"zzz", None)] * 70
    assert model_sort(tsim, case, 0, False, False) == [] and model_sort(tsim, case, 0, True, True) == list(range(70))
    # the prefix chain and the cnt tie at the chunk boundaries
    chain = [b"x" * k for k in range(21)]
    rng.shuffle(chain)
    case = [line_of(rng, k) for k in chain]
    assert [len(field_text(case, i)) for i in model_sort(tsim, case)] == list(range(21))
    ties = [b"aaaaaaab", b"aaaaaaa\0", b"aaaaaaa", b"a" * 14 + b"b", b"a" * 14 + b"\0", b"a" * 14]
    case = [line_of(rng, k) for k in ties * 3]
    got = [field_text(case, i) for i in model_sort(tsim, case, 0, True, False)]
    assert got == sorted(ties * 3, reverse=True)


@pytest.mark.parametrize("n,desc,all_lines,max_bytes", [(0, False, True, 0), (1, True, False, 0), (130, False, True, 0),
                                                        (130, True, False, 2), (1500, True, True, 0)])
def test_table_cut_index_and_gather(tsim, gsim, n, desc, all_lines, max_bytes):
    """the numeric sort's table, scan and cut over the sorted lines at several limits and capacities, the index rows, and the
    extract's gather model: every output byte written once, nothing outside"""
    rng = random.Random(100 + n)
    case = make_case(rng, n, 12, holes=True)
    order = model_sort(tsim, case, max_bytes, desc, all_lines)
    buf, ends, vval, vstart = table_of(tsim, case)
    nsel = len(order)
    a_lines, a_ends = (_u32 * max(nsel, 1))(*order), (_u64 * max(n, 1))(*ends)
    src_off, dst_off = 3, 5
    src_len = (src_off + len(buf) + 15) // 16 * 16
    src = bytes([0xEE]) * src_off + buf + bytes([0xEE]) * (src_len - src_off - len(buf))
    for limit in (0, 1, nsel // 2 + 1, nsel, nsel + 1):
        nout = tsim.lsosim_limited(nsel, limit)
        assert nout == (min(limit, nsel) if limit else nsel)
        cstart, coff, tw = (_u64 * max(nout, 1))(), (_u64 * (nout + 1))(), (_u32 * max(nout, 1))()
        tsim.lsosim_table(a_lines, a_ends, nout, n, cstart, coff, tw)
        assert list(tw)[:nout] == [1] * nout
        tsim.lsosim_scan(coff, nout)
        rows = [case[i][0] + bytes([DELIM]) for i in order[:nout]]
        need = sum(len(t) for t in rows)
        for r in (0, nout // 2, nout - 1) if nout else ():
            row, i = (_i64 * 6)(), order[r]
            assert tsim.lstsim_index_row(buf, len(buf), vval, vstart, i, cstart, coff, r, row) == 0
            t, f = case[i]
            st = ends[i] - len(t)
            assert list(row) == [i, st, len(t), coff[r]] + ([st + f[0], f[1]] if isinstance(f, tuple) else [-1, -1])
        for cap in (need, need - 1, len(rows[0]) if rows else 0, len(rows[0]) + 2 if rows else 0, 0):
            if cap < 0:
                continue
            want, k = b"", 0
            for t in rows:
                if len(want) + len(t) > cap:
                    break
                want += t
                k += 1
            res = (_u64 * 4)()
            tsim.lsosim_result(coff, nout, cap, res)
            assert list(res) == [nout, need, k, len(want)], (limit, cap, list(res))
            out_bytes = res[3]
            if out_bytes == 0:
                continue        # (the call launches no gather)
            dst_len = (dst_off + out_bytes + 15) // 16 * 16
            dst = (_u8 * dst_len)(*([FILL] * dst_len))
            reads, writes = (_u32 * max(src_len, 1))(), (_u32 * dst_len)()
            win, glo = _u64(), _u64()
            bad = gsim.lesim_gather(coff, cstart, nout, out_bytes, src_off, dst_off, DELIM, DELIM, src, src_len, dst, dst_len, reads,
                                    writes, ctypes.byref(win), ctypes.byref(glo))
            assert bad == 0, ("accesses outside the aligned extents", bad, n, limit, cap)
            got = bytes(dst)
            assert got[dst_off:dst_off + out_bytes] == want
            w = list(writes)
            assert w[dst_off:dst_off + out_bytes] == [1] * out_bytes, "every output byte exactly once"
            assert not any(w[:dst_off]) and not any(w[dst_off + out_bytes:])
            assert got[:dst_off] == bytes([FILL]) * dst_off and got[dst_off + out_bytes:] == bytes([FILL]) * (dst_len - dst_off - out_bytes)
