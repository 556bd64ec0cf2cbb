"""The line route by key (sre_hip_route_lines_by_key): the header declares the struct and the entry point, libsregex.so
exports it, the Python mirror has it, and the argument checks that need no device refuse what the header says.  No GPU
needed."""
import ctypes
import inspect
import os
import re

import sregex_amd as S
import harness

NAME = "sre_hip_route_lines_by_key"


def header():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        return f.read()


def test_header_declares_the_struct_and_the_entry_point():
    text = header()
    assert re.search(r"typedef struct \{\s*size_t nlines, nkeyed, nmembers;[^}]*size_t nselected;[^}]*size_t nbuckets;[^}]*"
                     r"size_t need_bytes, nwritten, out_bytes;\s*\} sre_hip_route_key_info_t;", text)
    assert re.search(r"int sre_hip_route_lines_by_key\(sre_hip_scanner_t \*sc, const void \*d_buf, size_t len, int delim,\s*"
                     r"const int \*groups, size_t ngroups, const sre_hip_keyset_t \*ks, int flags,\s*void \*d_out, size_t out_cap,\s*"
                     r"sre_int_t \*d_keyid, size_t keyid_cap,\s*sre_int_t \*d_index, size_t index_cap,\s*"
                     r"sre_int_t \*d_buckets, size_t buckets_cap,\s*sre_hip_route_key_info_t \*info, void \*hip_stream\);", text)


def test_the_not_offered_lists():
    text = header()
    lookup = text[text.index("Line lookup: the lines of d_buf"):text.index("SRE_API int sre_hip_lookup_lines")]
    assert "routing by dictionary" not in lookup and "sre_hip_route_lines_by_key" in lookup
    for still in ("every match of a line", "caseless keys", "Thompson and COUNT scanners", "stream sets"):
        assert still in lookup, still
    mine = text[text.index("Line route by key: the lines of d_buf"):text.index("SRE_API int sre_hip_route_lines_by_key")]
    assert "Not offered:" in mine
    own = " ".join(mine[mine.index("Not offered:"):].replace("*", " ").split())
    for missing in ("a separate output pointer per bucket", "grouping by the buffer's own keys in one call",
                    "that matches the lines twice", "ordering the buckets by anything but the dictionary id", "INVERT",
                    "caseless keys", "every match of a line", "Thompson and COUNT scanners", "stream sets"):
        assert missing in own, missing
    assert "2^32 - 1 lines" in " ".join(mine.replace("*", " ").split())          # the header states the bound


def test_library_exports_the_entry_point():
    lib = ctypes.CDLL(S.LIB_PATH)
    assert hasattr(lib, NAME)
    assert NAME in S.API and len(S.API[NAME][1]) == 18 and S.API[NAME][0] is ctypes.c_int
    assert S.RouteKeyInfo._fields == ("nlines", "nkeyed", "nmembers", "nselected", "nbuckets", "need_bytes", "nwritten", "out_bytes")


def test_the_mirror_has_the_call():
    sig = inspect.signature(S.Scanner.route_lines_by_key)
    assert list(sig.parameters) == ["self", "ptr", "length", "out_ptr", "out_cap", "groups", "keyset", "delim", "all_lines",
                                    "keyid_ptr", "keyid_cap", "index_ptr", "index_cap", "buckets_ptr", "buckets_cap", "hip_stream"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"delim": 0x0A, "all_lines": False, "keyid_ptr": None, "keyid_cap": 0, "index_ptr": None, "index_cap": 0,
                 "buckets_ptr": None, "buckets_cap": 0, "hip_stream": None}


def test_refusals_that_need_no_device():
    """Every one of these is refused in front of the first look at the scanner, the set or the device: sc and ks stand for
    objects here and are zeroed host memory that a call which got further would trip over (a set of 0 fields)."""
    lib = S.load_library()
    sc, ks = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    text = ctypes.create_string_buffer(b"k=a\nk=b\n")        # (never read)
    side = ctypes.create_string_buffer(256)
    arr = (ctypes.c_int * 1)(1)
    info = (ctypes.c_size_t * 8)(*([77] * 8))
    ok = dict(sc=ctypes.addressof(sc), buf=ctypes.addressof(text), delim=10, groups=arr, ngroups=1, ks=ctypes.addressof(ks), flags=0,
              out=(ctypes.addressof(side), 64), keyid=(None, 0), index=(None, 0), buckets=(None, 0))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sre_hip_route_lines_by_key(a["sc"], a["buf"], 8, a["delim"], a["groups"], a["ngroups"], a["ks"], a["flags"],
                                              a["out"][0], a["out"][1], a["keyid"][0], a["keyid"][1], a["index"][0], a["index"][1],
                                              a["buckets"][0], a["buckets"][1], info, None)
    assert call(ks=None) == -1
    for flags in (S.HIP_LINES_INVERT, S.HIP_LINES_INVERT | S.HIP_LINES_ALL, 4, 1 << 30):
        assert call(flags=flags) == -1, flags
    assert call(groups=None) == -1 and call(ngroups=0) == -1
    for name in ("out", "keyid", "index", "buckets"):
        assert call(**{name: (None, 3)}) == -1, name
    for delim in (-1, 256, 1000):
        assert call(delim=delim) == -1, delim
    assert call(sc=None) == -1 and call(buf=None) == -1
    assert call(out=(ctypes.addressof(text) + 2, 4)) == -1          # the output overlaps the buffer
    assert call(sc=None, ks=None, buf=None, groups=None) == -1
    assert list(info) == [77] * 8
