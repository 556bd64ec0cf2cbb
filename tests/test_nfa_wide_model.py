"""The wide bit-parallel form of a program (sregex_amd/csrc/sre_nfa_wide.cpp: sets of 64, 128 or 256 bits),
checked on the CPU through a test-only sequential model (tests/nfa_wide_sim.cpp) against the oracle: thread
sets decide Thompson exactly, and for Pike the first MATCH event and the clean position in front of it
bracket the reference's match — under every build option, on programs with more than 64 threads."""
import ctypes
import os
import random
import subprocess

import pytest

import sregex_amd as S
import harness

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_vp, _i64, _u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64

NO_MERGE, EXPLICIT_ANY, PLAIN, MIN_W2, MIN_W4 = 1, 2, 4, 8, 16
OPTIONS = [0, NO_MERGE, EXPLICIT_ANY, PLAIN, MIN_W2, MIN_W4, NO_MERGE | EXPLICIT_ANY | MIN_W2, PLAIN | MIN_W2]


@pytest.fixture(scope="module")
def wsim(lib):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libnfawidesim.so")
    srcs = [os.path.join(HERE, "nfa_wide_sim.cpp"), os.path.join(ROOT, "sregex_amd", "csrc", "sre_nfa_wide.cpp")]
    deps = srcs + [os.path.join(ROOT, "sregex_amd", "csrc", "sre_nfa_wide.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-o", so] + srcs +
                              ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "sregex_amd", "csrc")])
    L = ctypes.CDLL(so)
    L.wsim_build.restype = _vp
    L.wsim_build.argtypes = [_vp, ctypes.c_uint, ctypes.POINTER(ctypes.c_char_p)]
    L.wsim_free.argtypes = [_vp]
    L.wsim_info.argtypes = [_vp, ctypes.POINTER(_i64)]
    L.wsim_valid.argtypes = [_vp, ctypes.POINTER(_u64)]
    L.wsim_run.argtypes = [_vp, ctypes.c_char_p, _i64, ctypes.c_int, ctypes.POINTER(_i64)]
    L.wsim_walk_set.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.c_char_p, _i64, ctypes.c_uint32, ctypes.POINTER(_u64)]
    return L


def info(wsim, h):
    v = (_i64 * 8)()
    wsim.wsim_info(h, v)
    return dict(zip(["W", "nbits", "raw_bits", "plain", "nlut", "nassert", "implicit_any", "lds"], list(v)))


def build(wsim, prog, opts=0):
    why = ctypes.c_char_p()
    h = wsim.wsim_build(prog.h, opts, ctypes.byref(why))
    return h, (why.value.decode() if why.value else None)


def check(wsim, h, ora, prog, ncaps, data):
    """complaints of the wide form against the oracle on one subject"""
    out = (_i64 * 3)()
    wsim.wsim_run(h, bytes(data), len(data), 0, out)
    ev, clean, how = out[0], out[1], out[2]
    bad = []
    t = ora.thompson(prog)
    th = t.exec(data, True)
    t.close()
    if (ev >= 0) != (th == 0):
        bad.append(("thompson", ev, th))
    p = ora.pike(prog, ncaps)
    rc = p.exec(data, True, want_pending=False)
    ov = list(p.ovector)
    p.close()
    if (rc >= 0) != (ev >= 0):
        bad.append(("pike rc", ev, rc))
    if rc >= 0 and ev >= 0:
        # the match starts at or behind the clean position, and it ends where a thread reached MATCH: no
        # earlier than the first event (a consumed byte lists MATCH behind itself, an expansion at its position)
        if not (clean <= ov[0] and ov[1] >= ev + (1 if how == 0 else 0)):
            bad.append(("bracket", ev, how, clean, ov[:2]))
    return bad


def zoo():
    progs = []
    for k in (30, 31, 45, 60, 61, 62, 90, 120):
        progs.append([b"(?:a|b)*a(?:a|b){%d}@" % k])
    for k, m in ((20, 40), (40, 40), (60, 60), (100, 100), (110, 130), (40, 200)):
        progs.append([b"[ab]*a[ab]{%d}c[^x]{%d}@" % (k, m)])
    progs += [[b"[ab]*a[ab]{40}c[^x]{40}$"], [b"\\b[ab]*a[ab]{50}c[^x]{30}\\b"], [b"[ab]*a[ab]{70}c\\b"],
              [b"^[ab]*a[ab]{40}c[^x]{40}@"], [b"(?:^|x)[ab]*a[ab]{70}c"], [b"^x[^y\n]*y[ab]{80}"],
              [b"[ab]*a[ab]{40}c", b"[ab]*b[ab]{40}@", b"x[^y]*y[ab]{20}"],
              [b"x[^y]*y[ab]*a[ab]{40}c[^x]{40}@"], [b"x{100,}"], [b"x.{0,100}y"], [b"x.{0,300}y"],
              [b"(x|y|z[QW]){1,5}(longish|loooonger|evenlooooooonger|tiny){1,5}"]]
    return progs


def subjects(rng, alphabet, n):
    return [bytes(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 40, 130, 300, 700]))) for _ in range(n)]


def test_bits_are_counted_after_merging(wsim):
    want = {b"(?:a|b)*a(?:a|b){30}@": 1, b"[ab]*a[ab]{40}c[^x]{40}@": 2, b"[ab]*a[ab]{100}c[^x]{100}@": 4}
    for pat, W in want.items():
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, [pat]))
            h, why = build(wsim, prog)
            assert h, (pat, why)
            i = info(wsim, h)
            wsim.wsim_free(h)
            print(pat, i)
            assert i["W"] == W, (pat, i)
            assert i["lds"] <= 160 * 1024


def kernel_lds(i):
    """the LDS sre_k_nfa_wide asks for (sre_hip_nfa_wide.hip layout), counted from the form's parameters"""
    e = 8 * i["W"]
    nl = 0 if i["nlut"] == 0 else next(v for v in (1, 2, 4, 8, 16) if v >= i["nlut"])
    tile = 256 * (64 + 16) + 256 * 16
    return (tile + 256 * e + 256 * 4 + (256 * e if nl > i["nlut"] else 0) + i["nlut"] * 256 * e
            + ((16 << i["nassert"]) * e if i["nassert"] else 0))


def test_admitted_forms_fit_the_kernels_lds_at_the_boundary(wsim):
    """the builder admits a form only when what the kernel asks for fits one workgroup (160 KiB): long optional
    chains next to class runs sweep the lookup count across the budget"""
    admitted, declined = [], []
    pats = [b"x.{0,%d}y[ab]{60}c" % n for n in range(100, 127)]
    pats += [b"[ab]*a[ab]{60}cx.{0,%d}@" % n for n in range(96, 118)]
    pats += [b"[ab]*a[ab]{60}cx.{0,%d}\\b" % n for n in range(60, 90, 3)]
    for pat in pats:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, [pat]))
            for opts in (0, MIN_W4):
                h, why = build(wsim, prog, opts)
                if not h:
                    declined.append((pat, opts, why))
                    continue
                i = info(wsim, h)
                wsim.wsim_free(h)
                admitted.append((pat, opts, i["W"], i["nlut"], kernel_lds(i)))
                assert i["lds"] == kernel_lds(i), (pat, opts, i)
                assert kernel_lds(i) <= 160 * 1024, (pat, opts, i)
    print(max(a[-1] for a in admitted), len(admitted), len(declined))
    assert any(a[2] == 4 and a[4] > 150 * 1024 for a in admitted), admitted[-5:]
    assert any("LDS" in d[2] for d in declined), declined[:5]


def test_declines_what_it_cannot_hold(wsim):
    cases = {b"[ab]*a[ab]{150}c[^x]{150}@": "256", b"(?:a|b)*a(?:a|b){30}": None, b"a*": "nullable",
             b"x.{0,300}y.{0,300}z": None}
    for pat, word in cases.items():
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, [pat]))
            h, why = build(wsim, prog)
            if pat == b"(?:a|b)*a(?:a|b){30}":
                assert h, why           # (no trailing byte: still a form)
                wsim.wsim_free(h)
                continue
            assert not h, pat
            print(pat, why)
            if word:
                assert word in why, (pat, why)


def test_wide_form_vs_oracle_zoo_every_option(wsim):
    ora = harness.OracleEngine()
    rng = random.Random(int(os.environ.get("SRE_FUZZ_SEED", "20261004")) + 77)
    admitted, bad, wide = 0, [], set()
    for pats in zoo():
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            alphabet = b"abcx@y\n " if len(pats) > 1 or b"x" in pats[0] else b"ab@c"
            datas = subjects(rng, alphabet, 12)
            # subjects that hold a match of the bounded repetition
            datas += [bytes(rng.choice(b"ab") for _ in range(400)) + b"c" + b"z" * 250 + b"@",
                      b"x" * 120 + b"y" + bytes(rng.choice(b"ab") for _ in range(200)) + b"c" + b"\n" * 3]
            for opts in OPTIONS:
                h, why = build(wsim, prog, opts)
                if not h:
                    continue
                i = info(wsim, h)
                wide.add(i["W"])
                for d in datas:
                    r = check(wsim, h, ora, prog, re.ncaps, d)
                    admitted += 1
                    if r:
                        bad.append((pats, opts, d[:40], r))
                wsim.wsim_free(h)
    assert not bad, (len(bad), bad[:5])
    assert wide >= {1, 2, 4}, wide
    assert admitted > 1200, admitted


def test_wide_form_random_patterns_vs_oracle(wsim):
    """every program the builder takes, whatever its width (the narrow ones too: the same rules)"""
    ora = harness.OracleEngine()
    rng = random.Random(int(os.environ.get("SRE_FUZZ_SEED", "20261004")) + 78)
    alphabet = b"abcx \n_."
    admitted, bad = 0, []
    for it in range(900):
        nre = 1 if rng.random() < 0.8 else rng.randrange(2, 4)
        pats = [harness.random_regex(rng) for _ in range(nre)]
        with S.Pool() as pool:
            try:
                re = S.parse(pool, pats)
            except Exception:
                continue
            prog = S.compile(pool, re)
            h, why = build(wsim, prog, OPTIONS[it % len(OPTIONS)])
            if not h:
                continue
            for _ in range(4):
                d = bytes(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 7, 40, 130, 400])))
                r = check(wsim, h, ora, prog, re.ncaps, d)
                admitted += 1
                if r:
                    bad.append((pats, OPTIONS[it % len(OPTIONS)], d, r))
            wsim.wsim_free(h)
    assert admitted > 1500, admitted
    assert not bad, (len(bad), bad[:5])


def test_reference_blocks_with_many_threads(wsim, blocks):
    """the reference runs whose programs hold more than 64 list-able threads: sized, and correct where admitted"""
    ora = harness.OracleEngine()
    rows, bad = [], []
    for blk in blocks:
        subject = bytes.fromhex(blk["s"])
        for name, regexes, flags, multi, ref in harness.block_variants(blk):
            if ref["rc"] != 0:
                continue
            with S.Pool() as pool:
                prog = S.compile(pool, S.parse(pool, regexes, flags, multi))
                nthreads = sum(1 for line in prog.dump().splitlines()
                               if line.split()[1:2] and line.split()[1] in ("char", "in", "notin", "any", "match"))
                if nthreads <= 64:
                    continue
                h, why = build(wsim, prog)
                if h:
                    i = info(wsim, h)
                    rows.append((blk["name"], name, nthreads, "W=%d bits=%d luts=%d" % (i["W"], i["nbits"], i["nlut"])))
                    r = check(wsim, h, ora, prog, ref["ncaps"], subject)
                    if r:
                        bad.append((blk["name"], name, r))
                    wsim.wsim_free(h)
                else:
                    rows.append((blk["name"], name, nthreads, why))
    for r in rows:
        print(*r)
    assert rows
    assert not bad, bad


def test_a_segment_is_a_union_homomorphism_of_its_entry_set_at_w_words(wsim):
    """What the wide exact-entry pass rests on: F(B u M) = F(B) u U_{i in M} F({i}) at W words."""
    rng = random.Random(int(os.environ.get("SRE_FUZZ_SEED", "20261004")) + 79)
    alphabet = b"abcx \n_.y@"
    progs = zoo()[:16]
    n, bad = 0, []
    for pats in progs:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, pats))
            for opts in (0, PLAIN | MIN_W2, EXPLICIT_ANY | MIN_W4):
                h, why = build(wsim, prog, opts)
                if not h:
                    continue
                W = info(wsim, h)["W"]
                valid = (_u64 * 4)()
                wsim.wsim_valid(h, valid)
                vmask = sum(valid[i] << (64 * i) for i in range(4))

                def walk(m, seg, prev):
                    a = (_u64 * 4)(*[(m >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])
                    o = (_u64 * 4)()
                    wsim.wsim_walk_set(h, a, seg, len(seg), prev, o)
                    return sum(o[i] << (64 * i) for i in range(4))

                for _ in range(4):
                    seg = bytes(rng.choice(alphabet) for _ in range(rng.choice([1, 5, 64, 200])))
                    prev = rng.randrange(4)
                    B = rng.getrandbits(256) & vmask & rng.getrandbits(256)
                    M = rng.getrandbits(256) & vmask & rng.getrandbits(256) & rng.getrandbits(256)
                    whole = walk(B | M, seg, prev)
                    parts = walk(B, seg, prev)
                    for i in range(64 * W):
                        if (M >> i) & 1:
                            parts |= walk(1 << i, seg, prev)
                    n += 1
                    if whole != parts:
                        bad.append((pats, opts, seg[:30]))
                wsim.wsim_free(h)
    assert not bad, (len(bad), bad[:3])
    assert n > 100, n
