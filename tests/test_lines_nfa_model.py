"""A short line of line mode on the bit-parallel NFA tier, on the CPU: the step the short-line kernel
compiles (sregex_amd/csrc/sre_lines_nfa.h) walked over single lines (tests/lines_nfa_sim.cpp), against
the oracle and against the set model of the tier (tests/nfa_sim.cpp) run over the line as one stream."""
import ctypes
import os
import random
import subprocess

import pytest

import sregex_amd as S
import harness
from test_gpu_parity import NFA_ZOO
from test_nfa_model import SA_OPTIONS, sim as nfa_sim      # noqa: F401  (the fixture that builds tests/nfa_sim.cpp)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_vp, _i64 = ctypes.c_void_p, ctypes.c_int64
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 200]
ALPHABETS = [b"ab", b"ab@c", b"abcx ,.\n", b"a b\nc_x@y.", b"\xe7\xab\xa0\na"]
PLAIN, SA = 0, 1


@pytest.fixture(scope="module")
def lsim(lib):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "liblinesnfasim.so")
    csrc = os.path.join(ROOT, "sregex_amd", "csrc")
    srcs = [os.path.join(HERE, "lines_nfa_sim.cpp"), os.path.join(csrc, "sre_nfa.cpp")]
    deps = srcs + [os.path.join(csrc, h) for h in ("sre_nfa.h", "sre_lines_nfa.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-o", so] + srcs +
                              ["-I" + os.path.join(ROOT, "include"), "-I" + csrc])
    L = ctypes.CDLL(so)
    L.lnsim_build.restype = _vp
    L.lnsim_build.argtypes = [_vp, ctypes.c_uint, ctypes.POINTER(ctypes.c_char_p)]
    L.lnsim_free.argtypes = [_vp]
    L.lnsim_nfa.restype = _vp
    L.lnsim_nfa.argtypes = [_vp]
    L.lnsim_shape.argtypes = [_vp, ctypes.c_int]
    L.lnsim_walk.restype = _i64
    L.lnsim_walk.argtypes = [_vp, ctypes.c_int, ctypes.c_char_p, _i64]
    return L


def subjects(rng, pats):
    """random lines of every length over small alphabets, and lines that end in text the program matches"""
    out = []
    for n in LENGTHS:
        for alpha in ALPHABETS:
            out.append(bytes(rng.choice(alpha) for _ in range(n)))
    tails = [b"abaabaabab@", b"ab" * 8 + b"c", b"a,b,c,d", b"aa bb cc dd", b"x" + b"q" * 20 + b"x", b"ab", b"c", b"a b",
             b"\xe7\xab\xa0", b"xab ", b"a://b.c/d?e"]
    for n in LENGTHS:
        for t in tails:
            if len(t) <= n:
                out.append(bytes(rng.choice(b"ab ") for _ in range(n - len(t))) + t)
    return out


def set_model_event(nfa_sim, nfa, form, data):
    """the first event of the tier's set model over the line as one stream (an event at len(data): at the end of input)"""
    out = (_i64 * 3)()
    if form == SA:
        nfa_sim.nfa_sim_run_sa(nfa, bytes(data), len(data), 0, out)
        assert out[2] < 0, ("the two forms of the set model disagree", out[2])
    else:
        nfa_sim.nfa_sim_run(nfa, bytes(data), len(data), 0, out)
    return out[0]


def test_short_line_walk_equals_the_oracle_and_the_set_model(lsim, nfa_sim):
    ora = harness.OracleEngine()
    rng = random.Random(int(os.environ.get("SRE_FUZZ_SEED", "20261017")) + 11)
    shapes, admitted, compared, bad = set(), 0, 0, []
    for pats in NFA_ZOO:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, pats))
            lines = subjects(rng, pats)
            want = {}
            for opts in SA_OPTIONS + [128]:
                why = ctypes.c_char_p()
                h = lsim.lnsim_build(prog.h, opts, ctypes.byref(why))
                if not h:
                    continue
                admitted += 1
                nfa = lsim.lnsim_nfa(h)
                for form in (PLAIN, SA):
                    shape = lsim.lnsim_shape(h, form)
                    if shape < 0 or (form == PLAIN and opts not in (0, 128)):
                        continue        # (the plain form does not depend on the shift-and options)
                    shapes.add(shape)
                    for line in lines:
                        if line not in want:
                            t = ora.thompson(prog)
                            want[line] = t.exec(line, True) == S.SRE_OK
                            t.close()
                        ev = lsim.lnsim_walk(h, form, line, len(line))
                        compared += 1
                        if (ev >= 0) != want[line]:
                            bad.append((pats, opts, form, line, "oracle", ev, want[line]))
                        model = set_model_event(nfa_sim, nfa, form, line)
                        if ev != model:
                            bad.append((pats, opts, form, line, "set model", ev, model))
                lsim.lnsim_free(h)
    assert not bad, (len(bad), bad[:4])
    assert admitted >= len(NFA_ZOO), admitted           # every program of the zoo has a 64-bit form
    assert compared > 20000, compared
    # every table shape: plain / shift-and, each with and without look-ahead; and events from the consumed set
    assert {0, 1, 2, 3} <= shapes and 5 in shapes, shapes


def test_end_of_input_events_and_empty_lines(lsim, nfa_sim):
    """`c$` by hand: the event of a look-ahead program at the end of input is at the line's length, an empty line takes
    its EOF step, and the byte in front of a line's offset 0 is the start of the stream"""
    with S.Pool() as pool:
        for pat, line, ev in [(rb"c$", b"abc", 3), (rb"c$", b"abca", -1), (rb"c$", b"", -1), (rb"^(.*)$", b"", 0),
                              (rb"\bab\b", b"ab", 2), (rb"\bab\b", b"xab", -1), (rb"\bab\b", b" ab,", 3), (rb"(b)\z", b"ab", 2),
                              (rb"^b+", b"b", 0), (rb"^b+", b"ab", -1), (rb"^b+", b"a\nb", 2)]:
            prog = S.compile(pool, S.parse(pool, [pat]))
            why = ctypes.c_char_p()
            h = lsim.lnsim_build(prog.h, 0, ctypes.byref(why))
            assert h, (pat, why.value)
            for form in (PLAIN, SA):
                if lsim.lnsim_shape(h, form) >= 0:
                    assert lsim.lnsim_walk(h, form, line, len(line)) == ev, (pat, line, form)
                    assert set_model_event(nfa_sim, lsim.lnsim_nfa(h), form, line) == ev, (pat, line, form)
            lsim.lnsim_free(h)
