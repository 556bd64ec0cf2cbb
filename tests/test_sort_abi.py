"""The line sort (sre_hip_sort_lines): the header declares the flag, the struct and the entry point, libsregex.so exports it,
the Python mirror has it, and the argument checks that need no device refuse what the header says.  No GPU needed."""
import ctypes
import inspect
import os
import re

import sregex_amd as S
import harness

NAME = "sre_hip_sort_lines"
FIELDS = ("nlines", "nkeyed", "nnumbered", "nselected", "need_bytes", "nwritten", "out_bytes", "passes", "vmin", "vmax")


def header():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        return f.read()


def test_header_declares_the_flag_the_struct_and_the_entry_point():
    text = header()
    assert re.search(r"enum \{ SRE_HIP_SORT_DESC = 4 \};", text)
    assert re.search(r"typedef struct \{\s*size_t\s+nlines;[^}]*size_t\s+nkeyed;[^}]*size_t\s+nnumbered;[^}]*size_t\s+nselected;[^}]*"
                     r"size_t\s+need_bytes, nwritten, out_bytes;[^}]*size_t\s+passes;[^}]*int64_t\s+vmin, vmax;[^}]*"
                     r"\} sre_hip_sort_info_t;", text)
    assert re.search(r"int sre_hip_sort_lines\(sre_hip_scanner_t \*sc, const void \*d_buf, size_t len, int delim,\s*"
                     r"int group, int flags, size_t limit,\s*void \*d_out, size_t out_cap,\s*"
                     r"sre_int_t \*d_index, size_t index_cap,\s*sre_hip_sort_info_t \*info, void \*hip_stream\);", text)
    # the block stands behind the route by key's
    assert text.index("SRE_API int sre_hip_route_lines_by_key") < text.index("SRE_HIP_SORT_DESC") < text.index("stream sets: many")


def test_the_not_offered_list_and_the_rules_the_header_states():
    text = header()
    mine = text[text.index("Line sort: the lines of d_buf"):text.index("SRE_API int sre_hip_sort_lines")]
    flat = " ".join(mine.replace("*", " ").split())
    assert "Not offered:" in flat
    own = flat[flat.index("Not offered:"):]
    for missing in ("text or locale order", "floating point", "sort -u", "several columns in one call",
                    "sorting extracted fields instead of whole lines", "a per-line value array supplied by the caller", "INVERT",
                    "every match of a line", "Thompson and COUNT scanners", "stream sets"):
        assert missing in own, missing
    for stated in ("exactly those of sre_hip_lookup_lines", "sre_hip_tally_sums_lines", "stay in line order in BOTH directions",
                   "a second call on the output sorts by a second column", "those of sre_hip_route_lines", "2^32 - 1 lines",
                   "6 sre_int_t", "INT64_MAX / INT64_MIN"):
        assert stated in flat, stated
    # the rule is cited, not restated
    assert "1 to 18" not in flat and "an optional" not in flat.split("Index.")[0]


def test_library_exports_the_entry_point():
    lib = ctypes.CDLL(S.LIB_PATH)
    assert hasattr(lib, NAME)
    assert NAME in S.API and len(S.API[NAME][1]) == 13 and S.API[NAME][0] is ctypes.c_int
    assert S.SortInfo._fields == FIELDS
    assert S.HIP_SORT_DESC == 4 and S.HIP_SORT_DESC & (S.HIP_LINES_ALL | S.HIP_LINES_INVERT) == 0
    assert ctypes.sizeof(S.SortInfoStruct) == 8 * ctypes.sizeof(ctypes.c_size_t) + 16


def test_the_mirror_has_the_call():
    sig = inspect.signature(S.Scanner.sort_lines)
    assert list(sig.parameters) == ["self", "ptr", "length", "out_ptr", "out_cap", "group", "delim", "descending", "all_lines",
                                    "limit", "index_ptr", "index_cap", "hip_stream"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"delim": 0x0A, "descending": False, "all_lines": False, "limit": 0, "index_ptr": None, "index_cap": 0,
                 "hip_stream": None}


def test_refusals_that_need_no_device():
    """Every one of these is refused in front of the first look at the scanner or the device: sc stands for an object here and
    is zeroed host memory that a call which got further would trip over."""
    lib = S.load_library()
    sc = ctypes.create_string_buffer(4096)
    text = ctypes.create_string_buffer(b"v=1\nv=2\n")        # (never read)
    side = ctypes.create_string_buffer(256)
    info = S.SortInfoStruct(*([77] * 10))
    ok = dict(sc=ctypes.addressof(sc), buf=ctypes.addressof(text), delim=10, group=1, flags=0, limit=0,
              out=(ctypes.addressof(side), 64), index=(None, 0))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sre_hip_sort_lines(a["sc"], a["buf"], 8, a["delim"], a["group"], a["flags"], a["limit"], a["out"][0], a["out"][1],
                                      a["index"][0], a["index"][1], ctypes.byref(info), None)
    for flags in (S.HIP_LINES_INVERT, S.HIP_LINES_INVERT | S.HIP_LINES_ALL, 8, 1 << 30, S.HIP_SORT_DESC | 8,
                  S.HIP_SORT_DESC | S.HIP_LINES_INVERT):
        assert call(flags=flags) == -1, flags
    for name in ("out", "index"):
        assert call(**{name: (None, 3)}) == -1, name
    for delim in (-1, 256, 1000):
        assert call(delim=delim) == -1, delim
    assert call(sc=None) == -1 and call(buf=None) == -1
    assert call(sc=None, flags=S.HIP_SORT_DESC | S.HIP_LINES_ALL, limit=5) == -1
    assert call(out=(ctypes.addressof(text) + 2, 4)) == -1          # the output overlaps the buffer
    assert call(sc=None, buf=None, out=(None, 3)) == -1
    assert [getattr(info, f) for f in FIELDS] == [77] * 10
