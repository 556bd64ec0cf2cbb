"""Stream sets on the NFA tier (sre_hip_streams_create_engine): the header declares the new entry points,
libsregex.so exports them, the Python mirror takes the engine.  No GPU needed."""
import ctypes
import inspect
import os
import re

import sregex_amd as S
import harness

NAMES = ["sre_hip_streams_create_engine", "sre_hip_streams_engine", "sre_hip_streams_nfa_bits",
         "sre_hip_streams_last_exact_passes"]


def test_header_declares_the_new_entry_points():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        text = f.read()
    for name in NAMES:
        assert re.search(r"SRE_API\s+[\w \*]+\b%s\s*\(" % name, text), name
    assert re.search(r"sre_hip_streams_create_engine\s*\(\s*sre_pool_t \*pool,\s*sre_program_t \*prog,\s*int mode,\s*int engine,"
                     r"\s*size_t nstreams\)", text)


def test_library_exports_the_new_entry_points():
    lib = ctypes.CDLL(S.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in S.API, name
    assert S.API["sre_hip_streams_create_engine"][1][2:] == [ctypes.c_int, ctypes.c_int, ctypes.c_size_t]


def test_stream_set_takes_an_engine():
    sig = inspect.signature(S.StreamSet.__init__)
    assert list(sig.parameters) == ["self", "pool", "prog", "mode", "nstreams", "engine"]
    assert sig.parameters["engine"].default is None
    for attr in ("engine", "nfa_bits", "last_exact_passes"):
        assert isinstance(getattr(S.StreamSet, attr), property), attr


def test_the_rule_header_is_shared_by_the_device_tail_and_the_model():
    csrc = os.path.join(harness.ROOT, "sregex_amd", "csrc")
    for path in (os.path.join(csrc, "sre_hip_streams.hip"), os.path.join(harness.ROOT, "tests", "streams_nfa_sim.cpp")):
        with open(path) as f:
            text = f.read()
        assert '#include "sre_streams_nfa.h"' in text and "sre_streams_nfa_rule(" in text, path
