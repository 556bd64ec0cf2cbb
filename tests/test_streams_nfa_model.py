"""A stream of a stream set on the bit-parallel NFA tier, on the CPU: the rule of one call
(sregex_amd/csrc/sre_streams_nfa.h — the text the device tail compiles) around a sequential walk of the
thread set (tests/streams_nfa_sim.cpp), fed chunk by chunk, against the oracle's Thompson context fed the
same calls.  Every form the tier runs: the plain slices, the shift-and form under every build option, the
wide form at 1, 2 and 4 words."""
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
SEED = int(os.environ.get("SRE_FUZZ_SEED", "20261017"))

PLAIN, SA, WIDE = 0, 1, 2
SA_MASKED, SA_EVACC, SA_W64, SA_CARRY, SA_NO_MERGE, SA_EXPLICIT_ANY, SA_NO_EVACC = 1, 2, 4, 8, 16, 32, 64
SA_OPTIONS = [0, SA_MASKED, SA_EVACC, SA_NO_EVACC, SA_W64, SA_W64 | SA_CARRY, SA_NO_MERGE | SA_EXPLICIT_ANY,
              SA_MASKED | SA_EVACC | SA_W64 | SA_CARRY, SA_NO_EVACC | SA_W64 | SA_EXPLICIT_ANY]
WIDE_MIN_W2, WIDE_MIN_W4 = 8, 16
FORMS = [(PLAIN, 0)] + [(SA, o) for o in SA_OPTIONS] + [(WIDE, 0), (WIDE, WIDE_MIN_W2), (WIDE, WIDE_MIN_W4)]
SIZES = [0, 1, 7, 64, 255, 256, 1000]       # the schedule() of test_gpu_streams.py, at this model's subject sizes

OPEN, CLOSED, WAS_CLOSED, NOT_FED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def sim(lib):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libstreamsnfasim.so")
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    srcs = [os.path.join(HERE, "streams_nfa_sim.cpp"), os.path.join(csrc, "sre_nfa.cpp"), os.path.join(csrc, "sre_nfa_wide.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("sre_nfa.h", "sre_nfa_wide.h", "sre_streams_nfa.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-o", so] + srcs +
                              ["-I" + os.path.join(ROOT, "include"), "-I" + csrc])
    L = ctypes.CDLL(so)
    L.snsim_build.restype = _vp
    L.snsim_build.argtypes = [_vp, ctypes.c_int, ctypes.c_uint, ctypes.POINTER(ctypes.c_char_p)]
    L.snsim_free.argtypes = [_vp]
    L.snsim_words.argtypes = [_vp]
    L.snsim_call.argtypes = [_vp, ctypes.POINTER(_u64), ctypes.c_char_p, _i64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_i64)]
    return L


def build_forms(sim, prog):
    """[(kind, options, handle, words)] of every form the program has"""
    out = []
    for kind, opts in FORMS:
        why = ctypes.c_char_p()
        h = sim.snsim_build(prog.h, kind, opts, ctypes.byref(why))
        if h:
            out.append((kind, opts, h, sim.snsim_words(h)))
    return out


class ModelStream:
    def __init__(self, sim, h):
        self.sim, self.h = sim, h
        self.row = (_u64 * 5)()

    def call(self, chunk, eof, fed=True):
        out = (_i64 * 3)()
        self.sim.snsim_call(self.h, self.row, bytes(chunk), len(chunk), 1 if eof else 0, 1 if fed else 0, out)
        return out[0], out[1]


class OracleStream:
    """the oracle's Thompson context fed the calls; a closed stream repeats its closing rc (state 2)"""

    def __init__(self, ora, prog):
        self.ctx = ora.thompson(prog)
        self.closed = None

    def call(self, chunk, eof):
        if self.closed is not None:
            return self.closed, WAS_CLOSED
        rc = self.ctx.exec(bytes(chunk), eof)
        if rc == S.SRE_AGAIN:
            return rc, OPEN
        self.closed = rc
        self.ctx.close()
        return rc, CLOSED

    def close(self):
        if self.closed is None:
            self.ctx.close()


def first_event(ora, prog, data):
    """the byte whose step lists MATCH, from the oracle fed a byte a call (-1: none)"""
    o = ora.thompson(prog)
    ev = -1
    for p in range(len(data)):
        if o.exec(data[p:p + 1], False) == S.SRE_OK:
            ev = p - 1
            break
    else:
        if o.exec(b"", True) == S.SRE_OK:
            ev = len(data) - 1
    o.close()
    return ev


def cut(data, points, eof_last=True):
    """[(chunk, eof)] of data cut at the sorted offsets `points` (equal offsets: an empty chunk)"""
    edges = [0] + list(points) + [len(data)]
    calls = [(data[a:b], False) for a, b in zip(edges, edges[1:])]
    if eof_last:
        calls[-1] = (calls[-1][0], True)
    return calls


def schedules(rng, ora, prog, data):
    """call sequences of one subject: tiny calls, the schedule() style, and every way of cutting at the match"""
    out = []
    pts, o = [], 0
    while o < len(data):
        o = min(len(data), o + rng.randrange(0, 21))
        pts.append(o)
    out.append(cut(data, pts[:-1]))
    pts, o = [], 0
    for _ in range(rng.randrange(0, 9)):
        o = min(len(data), o + rng.choice(SIZES))
        pts.append(o)
    out.append(cut(data, pts))
    ev = first_event(ora, prog, data)
    if ev >= 0:
        e = ev + 1                      # the chunk [.., e) ends in the byte that lists MATCH: the match is pending
        out.append(cut(data, [e]))                      # the match at the last byte of a chunk
        out.append(cut(data, [ev]))                     # ... at the first byte of the next
        out.append(cut(data, [e, e]))                   # an empty chunk behind the pending match
        out.append(cut(data, [e, e, e]))
        out.append(cut(data, [e - 1, e - 1, e, e]))     # empty chunks in front of and behind it
        out.append(cut(data[:e], []))                   # the stream ends in the match: eof meets it
        out.append(cut(data[:e], [e]))                  # ... or an empty eof call does
        out.append(cut(data[:e], [e, e]))
        out.append(cut(data, [0, 0, e]))                # empty calls on a fresh stream
    else:
        out.append(cut(data, [0, 0, len(data) // 2, len(data) // 2, len(data)]))
    return out


def run_program(sim, ora, rng, prog, subjects, need):
    """-> (generated, compared, complaints) over every form of the program; `need`: kinds that must exist"""
    forms = build_forms(sim, prog)
    kinds = {f[0] for f in forms}
    assert need <= kinds, (need, kinds)
    generated = compared = 0
    bad = []
    for data in subjects:
        for calls in schedules(rng, ora, prog, data):
            calls = calls + [(b"zz", False)]            # one more call: a closed stream repeats, an open one goes on
            o = OracleStream(ora, prog)
            want = [o.call(c, e) for c, e in calls]
            o.close()
            for kind, opts, h, W in forms:
                m = ModelStream(sim, h)
                assert m.call(b"", False, fed=False)[1] == NOT_FED      # an idle call changes nothing
                first_bad = None
                for i, (c, e) in enumerate(calls):
                    generated += 1
                    got = m.call(c, e)
                    compared += 1
                    if got != want[i] and first_bad is None:
                        first_bad = (kind, opts, W, data[:60], [(len(x), y) for x, y in calls], i, got, want[i])
                if first_bad:
                    bad.append(first_bad)
    for f in forms:
        sim.snsim_free(f[2])
    return generated, compared, bad, forms


def rand_text(rng, alphabet, n):
    return bytes(rng.choice(alphabet) for _ in range(n))


# program, subjects with a match (beside random text), forms that must exist
def zoo(rng):
    ab = lambda n: rand_text(rng, b"ab", n)
    return [
        (rb"(?:a|b)*a(?:a|b){7}@", [ab(90) + b"ba" * 9 + b"@" + ab(30), b"ab@" + ab(40)], {PLAIN, SA, WIDE}),
        (rb"(?:a|b)*a[ab]{20}c[^x]{30}@", [ab(50) + b"a" + ab(20) + b"c" + b"\n" * 30 + b"@ab", ab(70) + b"c" + b"y" * 30 + b"@"], {PLAIN, SA, WIDE}),
        (rb"[ab]*a[ab]{45}c[^x]{45}@", [ab(130) + b"c" + b"@" * 46 + ab(9), b"x" + ab(46) + b"a" * 46 + b"c" + b"c" * 45 + b"@"], {WIDE}),
        (rb"(?:a|b)*a(?:a|b){30}@", [ab(100) + b"@" + ab(10), b"@@" + b"ba" * 20 + b"@"], {WIDE}),
        (rb"[ab]*a[ab]{95}c[^x]{95}@", [ab(200) + b"c" + b"y" * 95 + b"@" + ab(5)], {WIDE}),
        (rb"(?:a|b)*a(?:a|b){60}@", [ab(140) + b"@" + ab(10)], {WIDE}),
        (rb"x{20,56}y", [b"ab" + b"x" * 30 + b"y" + b"x" * 10, b"x" * 19 + b"y" + b"x" * 57 + b"y"], {PLAIN}),
        # ^ in the program (tools/nfa_layout_probe.py: both have a plain and a shift-and form)
        (rb"^[ab]*a[ab]{20}@", [b"xx\n" + ab(40) + b"@", b"x" + ab(30) + b"@\n" + ab(25) + b"@", ab(22) + b"@"], {PLAIN, SA}),
        (rb"(?:^|x)[ab]*a[ab]{30}c", [b"cc\n" + ab(50) + b"c", b"y" + ab(40) + b"c" + b"x" + ab(35) + b"c"], {PLAIN, SA}),
        # anchored: the set dies with the first byte that does not fit
        (rb"\Aab(?:a|b){30}c", [b"ab" + ab(30) + b"c" + ab(10), b"ab" + ab(29) + b"c" + ab(10), b"b" + b"ab" + ab(30) + b"c"], {WIDE}),
    ]


def test_the_zoo_in_chunks_equals_the_oracle_in_every_form(sim):
    ora = harness.OracleEngine()
    rng = random.Random(SEED + 1)
    generated = compared = 0
    widths, kinds_seen = set(), set()
    for pat, hits, need in zoo(rng):
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, [pat]))
            subjects = list(hits) + [rand_text(rng, b"ab@cx\n", n) for n in (0, 1, 130, 400)]
            g, c, bad, forms = run_program(sim, ora, rng, prog, subjects, need)
            assert not bad, (pat, len(bad), bad[:3])
            generated += g
            compared += c
            widths |= {f[3] for f in forms if f[0] == WIDE}
            kinds_seen |= {(f[0], f[1]) for f in forms}
    assert compared == generated and generated > 10000, (compared, generated)        # no case skipped
    assert widths >= {1, 2, 4}, widths
    assert kinds_seen == set(FORMS), set(FORMS) - kinds_seen


def test_matches_on_chunk_boundaries_close_or_stay_pending(sim):
    """the pending flag by hand: `ab@` ends chunk 1 -> AGAIN; an empty call keeps it pending; any call that runs
    a position answers OK; a closed stream repeats OK and reads nothing"""
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [rb"(?:a|b)*a(?:a|b){7}@"]))
        for kind, opts, h, W in build_forms(sim, prog):
            m = ModelStream(sim, h)
            assert m.call(b"", False) == (S.SRE_AGAIN, OPEN)
            assert m.call(b"xxab" + b"ab" * 4 + b"@", False) == (S.SRE_AGAIN, OPEN), (kind, opts)
            assert m.call(b"", False) == (S.SRE_AGAIN, OPEN)
            assert m.call(b"", False, fed=False)[1] == NOT_FED
            assert m.call(b"q", False) == (S.SRE_OK, CLOSED), (kind, opts)
            assert m.call(b"anything", True) == (S.SRE_OK, WAS_CLOSED)
            m = ModelStream(sim, h)
            assert m.call(b"ab" * 5 + b"@", False) == (S.SRE_AGAIN, OPEN)
            assert m.call(b"", True) == (S.SRE_OK, CLOSED), (kind, opts)
            m = ModelStream(sim, h)
            assert m.call(b"ab" * 5, False) == (S.SRE_AGAIN, OPEN)
            assert m.call(b"", True) == (S.SRE_DECLINED, CLOSED)
            assert m.call(b"ab" * 5 + b"@", True) == (S.SRE_DECLINED, WAS_CLOSED)
            sim.snsim_free(h)


@pytest.mark.parametrize("seed", [SEED, SEED + 1000])
def test_random_programs_in_chunks_equal_the_oracle(sim, seed):
    """150 random look-ahead-free patterns per seed that the builder admits, every form of each"""
    ora = harness.OracleEngine()
    rng = random.Random(seed + 2)
    alphabet = b"abcx \n_."
    admitted = generated = compared = 0
    bad = []
    tries = 0
    while admitted < 150:
        tries += 1
        assert tries < 5000, admitted
        nre = 1 if rng.random() < 0.8 else rng.randrange(2, 4)
        pats = [harness.random_regex(rng) for _ in range(nre)]
        with S.Pool() as pool:
            try:
                re = S.parse(pool, pats)
            except Exception:
                continue
            prog = S.compile(pool, re)
            forms = build_forms(sim, prog)
            for f in forms:
                sim.snsim_free(f[2])
            if not forms:
                continue
            admitted += 1
            subjects = [rand_text(rng, alphabet, n) for n in (rng.choice([0, 1, 7]), 40, rng.choice([130, 400]))]
            g, c, b, _ = run_program(sim, ora, rng, prog, subjects, set())
            generated += g
            compared += c
            bad += [(pats,) + x for x in b]
    assert not bad, (len(bad), bad[:3])
    assert compared == generated and generated > 10000, (compared, generated)
