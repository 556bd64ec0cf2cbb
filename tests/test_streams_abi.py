"""Stream sets (sre_hip_streams_*): the header declares the entry points, libsregex.so exports
them and the Python mirror has its StreamSet class.  No GPU needed."""
import ctypes
import os
import re

import sregex_amd as S
import harness

NAMES = ["sre_hip_streams_create", "sre_hip_streams_count", "sre_hip_streams_result_slots",
         "sre_hip_streams_device_bytes", "sre_hip_streams_feed", "sre_hip_streams_reset",
         "sre_hip_streams_last_fixups", "sre_hip_streams_last_launches"]


def test_header_declares_the_stream_set_entry_points():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        text = f.read()
    assert "typedef struct sre_hip_streams_s sre_hip_streams_t;" in text
    for name in NAMES:
        assert re.search(r"SRE_API\s+[\w \*]+\b%s\s*\(" % name, text), name


def test_library_exports_the_stream_set_entry_points():
    lib = ctypes.CDLL(S.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in S.API, name


def test_python_mirror_has_a_stream_set_class():
    assert isinstance(S.StreamSet, type)
    for attr in ("feed", "reset", "device_bytes", "last_fixups", "last_launches"):
        assert hasattr(S.StreamSet, attr), attr
