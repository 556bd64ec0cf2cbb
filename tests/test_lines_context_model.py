"""The context pass of the line filter (sre_hip_filter_lines_context) on the CPU: tests/lines_context_sim.cpp runs marks,
carry and apply workgroup by workgroup with the block logic the kernels compile (sregex_amd/csrc/sre_lines_context.h)
and the kernels' 1024 / 256 / 64 geometry.  Expected: a dilation in Python, checked itself against the definition
(some matched j with j < i <= j + after or i < j <= i + before) on the small sizes."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_u64, _u32 = ctypes.c_uint64, ctypes.c_uint32
_p64, _p32 = ctypes.POINTER(_u64), ctypes.POINTER(_u32)
SIZE_MAX = (1 << 64) - 1
NONE = SIZE_MAX
CONTEXT, GROUP, SELECTED = 1, 2, 4
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 17]


@pytest.fixture(scope="module")
def csim():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "liblinescontextsim.so")
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    deps = [os.path.join(HERE, "lines_context_sim.cpp"), os.path.join(csrc, "sre_lines_context.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, deps[0], "-I" + csrc])
    L = ctypes.CDLL(so)
    L.lcsim_items.restype = _u32
    L.lcsim_run.restype = _u64
    L.lcsim_run.argtypes = [_p64, _p64, _u64, _u64, _u64, _p64, _p64, _p64]
    L.lcsim_carry.restype = None
    L.lcsim_carry.argtypes = [_p64, _p64, _u64]
    L.lcsim_block.restype = None
    L.lcsim_block.argtypes = [_p64, _u64, _u64, _u64, _u64, _u64, _u64, _p32]
    assert L.lcsim_items() == 1024
    return L


def windows(n):
    return [0, 1, 3, 4, 63, 64, 255, 256, 1023, 1024, 1025, max(n - 1, 0), n, n + 1, 1 << 63, SIZE_MAX]


def pairs(n, full):
    w = windows(n)
    if not full:
        return [(0, 0), (1, 1), (3, 0), (0, 4), (64, 63), (n - 1, n), (1 << 63, 0), (0, SIZE_MAX), (SIZE_MAX, SIZE_MAX)]
    out = [(x, x) for x in w] + [(x, 0) for x in w[1:]] + [(0, x) for x in w[1:]]
    out += [(1, 3), (4, 1), (63, 256), (255, 64), (1025, 3), (3, 1023), (n, 1), (1, n + 1), (1 << 63, 4), (255, SIZE_MAX)]
    return out


def dilate(matched, before, after):
    """the selected lines, from the nearest matched line at or in front of each line and at or behind it"""
    n = len(matched)
    p, q, last = [None] * n, [None] * n, None
    for i in range(n):
        last = i if matched[i] else last
        p[i] = last
    last = None
    for i in reversed(range(n)):
        last = i if matched[i] else last
        q[i] = last
    return [(p[i] is not None and i - p[i] <= after) or (q[i] is not None and q[i] - i <= before) for i in range(n)]


def by_definition(matched, before, after):
    js = [j for j, m in enumerate(matched) if m]
    return [matched[i] or any(j < i <= j + after or i < j <= i + before for j in js) for i in range(len(matched))]


def line_lengths(n, seed):
    rng = random.Random(seed)
    lens = [rng.randrange(0, 41) for _ in range(n)]
    ends, pos = [], 0
    for k in lens:
        ends.append(pos + k)
        pos += k + 1
    return lens, ends


def run(csim, matched, lens, ends, before, after, order=None):
    """the model over one set of matched lines; asserts everything it writes; returns the selected set"""
    n = len(matched)
    nblk = (n + 1023) // 1024
    val = (_u64 * n)(*[k + 1 if m else 0 for k, m in zip(lens, matched)])
    bits = (_u64 * ((n + 63) // 64))(*([SIZE_MAX] * ((n + 63) // 64)))
    counts = (_u64 * 2)()
    order = list(range(nblk)) if order is None else order
    bad = csim.lcsim_run(val, (_u64 * n)(*ends), n, before, after, (_u64 * nblk)(*order), bits, counts)
    ctx = (n, before, after, [i for i, m in enumerate(matched) if m][:8])
    assert bad == 0, ("apply touched val outside its workgroup", bad, ctx)
    sel = dilate(matched, before, after)
    assert list(val) == [k + 1 if s else 0 for k, s in zip(lens, sel)], ctx
    want_bits = [0] * ((n + 63) // 64)
    for i in range(n):
        if sel[i] and not matched[i]:
            want_bits[i // 64] |= 1 << (i % 64)
    assert list(bits) == want_bits, ctx
    groups = sum(1 for i in range(n) if sel[i] and (i == 0 or not sel[i - 1]))
    assert (counts[0], counts[1]) == (sum(matched), groups), ctx
    return sel


def plants(n):
    """matched lines at the edges of the buffer, of the waves and of the workgroups, alone and in pairs"""
    spots = [s for s in (0, n - 1, 255, 256, 1023, 1024) if 0 <= s < n]
    sets = [[s] for s in spots] + [[0, n - 1], [255, 256], [1023, 1024], [0, 1024], [255, n - 1], spots]
    out = []
    for s in sets:
        s = sorted({x for x in s if x < n})
        if s and s not in out:
            out.append(s)
    return out


def test_the_python_dilation_is_the_definition():
    rng = random.Random(3)
    for n in (1, 2, 5, 63, 65):
        for _ in range(12):
            m = [rng.random() < rng.choice([0.05, 0.5]) for _ in range(n)]
            for b, a in pairs(n, False) + [(2, 5), (5, 2)]:
                assert dilate(m, b, a) == by_definition(m, b, a)


@pytest.mark.parametrize("n", SIZES)
def test_planted_matches(csim, n):
    lens, ends = line_lengths(n, n)
    full = n in (65, 1025, 3 * 1024 + 17)
    for spots in plants(n):
        m = [False] * n
        for s in spots:
            m[s] = True
        for b, a in pairs(n, full and len(spots) <= 2):
            run(csim, m, lens, ends, b, a)


@pytest.mark.parametrize("n", SIZES)
def test_none_all_and_random_densities(csim, n):
    lens, ends = line_lengths(n, 100 + n)
    rng = random.Random(200 + n)
    for b, a in pairs(n, False):
        assert not any(run(csim, [False] * n, lens, ends, b, a))
        assert all(run(csim, [True] * n, lens, ends, b, a))
    for density in (1 / 2, 1 / 50, 1 / 2000):
        m = [rng.random() < density for _ in range(n)]
        for b, a in pairs(n, n == 3 * 1024 + 17 and density != 1 / 2):
            run(csim, m, lens, ends, b, a)


def test_carry_through_a_workgroup_without_a_match(csim):
    n = 3 * 1024 + 17
    lens, ends = line_lengths(n, 7)
    m = [False] * n
    m[5] = True
    sel = run(csim, m, lens, ends, 0, 2500)
    assert sel[1024:2048] == [True] * 1024 and sel[2505] and not sel[2506] and sum(sel) == 2501
    m = [False] * n
    m[n - 3] = True
    sel = run(csim, m, lens, ends, 2500, 0)
    assert sel[1024:2048] == [True] * 1024 and sel[n - 3 - 2500] and not sel[n - 3 - 2501] and not sel[n - 2]
    # two of them, contexts that just meet and just do not
    m = [False] * n
    m[5] = m[3000] = True
    for b, a, groups in [(1500, 1494, 1), (1500, 1493, 2), (0, 2994, 1), (2994, 0, 1), (1, 2992, 2)]:
        sel = run(csim, m, lens, ends, b, a)
        assert sum(1 for i in range(n) if sel[i] and (i == 0 or not sel[i - 1])) == groups, (b, a)


def test_apply_in_any_order_of_the_workgroups(csim):
    """in place: a workgroup reads no value another one writes, so the order of the workgroups changes nothing"""
    n = 5 * 1024 + 300
    lens, ends = line_lengths(n, 9)
    rng = random.Random(10)
    m = [rng.random() < 1 / 300 for _ in range(n)]
    for b, a in [(3, 3), (0, 1200), (1200, 0), (1024, 1024), (SIZE_MAX, 0)]:
        want = run(csim, m, lens, ends, b, a)
        for order in ([5, 4, 3, 2, 1, 0], [3, 0, 5, 1, 4, 2]):
            assert run(csim, m, lens, ends, b, a, order) == want


def test_carry_scan_of_many_blocks_and_64_bit_words(csim):
    """more block words than the carry's 1024 lanes (a run of several per lane), with line indices beyond 2^32"""
    rng = random.Random(11)
    for nblk in (1, 2, 64, 65, 1024, 1025, 5000):
        for density in (1.0, 0.3, 0.002):
            last, first = [], []
            for b in range(nblk):
                base = (b << 10) + (7 << 32)
                if rng.random() < density:
                    lo, hi = sorted((rng.randrange(1024), rng.randrange(1024)))
                    last.append(base + hi + 1)
                    first.append(base + lo)
                else:
                    last.append(0)
                    first.append(NONE)
            a_last, a_first = (_u64 * nblk)(*last), (_u64 * nblk)(*first)
            csim.lcsim_carry(a_last, a_first, nblk)
            pin, run_p = [], 0
            for x in last:
                pin.append(run_p)
                run_p = max(run_p, x)
            qin, run_q = [], NONE
            for x in reversed(first):
                qin.append(run_q)
                run_q = min(run_q, x)
            assert list(a_last) == pin and list(a_first) == qin[::-1], (nblk, density)


def test_one_workgroup_beyond_2_to_the_32(csim):
    """the arithmetic of apply with synthetic line indices: a workgroup far into a buffer of more than 2^32 lines, its
    carries given; Python integers say what is selected"""
    rng = random.Random(12)
    base = (5 << 32) + 3 * 1024
    cases = []
    for n in (base + 1024, base + 1000, base + 40 * 1024):
        for spots in ([], [0], [1023], [17, 600], [255, 256, 999]):
            for pin_at in (None, base - 1, base - 300, (1 << 32) + 5, 3):
                for qin_at in (None, base + 1024, base + 5000):
                    if qin_at is not None and qin_at >= n:
                        continue
                    cases.append((n, spots, pin_at, qin_at))
    windows_ = [0, 1, 299, 300, 1024, 4000, (4 << 32) + 3 * 1024 - 5, (4 << 32) + 3 * 1024 - 4, 1 << 63, SIZE_MAX]
    for n, spots, pin_at, qin_at in cases:
        v = [0] * 1024
        for s in spots:
            if base + s < n:
                v[s] = 9
        for _ in range(3):
            b, a = rng.choice(windows_), rng.choice(windows_)
            fl = (_u32 * 1024)()
            csim.lcsim_block((_u64 * 1024)(*v), base, n, 0 if pin_at is None else pin_at + 1, NONE if qin_at is None else qin_at,
                             b, a, fl)

            def selected(i):
                ps = [base + s for s in range(1024) if v[s] and base + s <= i] + ([pin_at] if pin_at is not None else [])
                qs = [base + s for s in range(1024) if v[s] and base + s >= i] + ([qin_at] if qin_at is not None else [])
                return i < n and ((bool(ps) and i - max(ps) <= a) or (bool(qs) and min(qs) - i <= b))

            for k in (0, 1, 2, 16, 17, 18, 254, 255, 256, 257, 299, 300, 301, 599, 600, 601, 998, 999, 1000, 1022, 1023):
                i = base + k
                want = 0
                if selected(i):
                    pred = selected(i - 1)
                    want = SELECTED | (0 if v[k] else CONTEXT) | (0 if pred else GROUP)
                assert fl[k] == want, (n - base, spots, pin_at, qin_at, b, a, k, fl[k], want)
