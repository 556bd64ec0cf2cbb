"""The line sort by text (sre_hip_sort_lines_text): the header declares the struct and the entry points, libsregex.so exports
them, the Python mirror has them, the argument checks that need no device refuse what the header says with info untouched, the
plan is the same list on both sides, and sre_hip_sort_lines is what it was.  No GPU needed."""
import ctypes
import inspect
import os
import re

import sregex_amd as S
import harness

NAME = "sre_hip_sort_lines_text"
FIELDS = ("nlines", "nkeyed", "nselected", "need_bytes", "nwritten", "out_bytes", "passes", "minlen", "maxlen")


def header():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        return f.read()


def test_header_declares_the_struct_and_the_entry_points():
    text = header()
    assert re.search(r"typedef struct \{\s*size_t\s+nlines;[^}]*size_t\s+nkeyed;[^}]*size_t\s+nselected;[^}]*"
                     r"size_t\s+need_bytes, nwritten, out_bytes;[^}]*size_t\s+passes;[^}]*size_t\s+minlen, maxlen;[^}]*"
                     r"\} sre_hip_sort_text_info_t;", text)
    assert re.search(r"int sre_hip_sort_lines_text\(sre_hip_scanner_t \*sc, const void \*d_buf, size_t len, int delim,\s*"
                     r"int group, size_t max_bytes, int flags, size_t limit,\s*void \*d_out, size_t out_cap,\s*"
                     r"sre_int_t \*d_index, size_t index_cap,\s*sre_hip_sort_text_info_t \*info, void \*hip_stream\);", text)
    assert re.search(r"size_t sre_hip_sort_text_plan\(size_t minlen, size_t maxlen, int rest, uint64_t \*pairs, size_t cap\);", text)
    # the block stands behind the ordered tally's
    assert text.index("SRE_API int sre_hip_tally_top_lines") < text.index("sre_hip_sort_text_info_t") < text.index("stream sets: many")


def test_the_not_offered_list_and_the_rules_the_header_states():
    text = header()
    mine = text[text.index("Line sort by text: the lines of d_buf"):text.index("SRE_API int sre_hip_sort_lines_text")]
    flat = " ".join(mine.replace("*", " ").split())
    assert "Not offered:" in flat
    own = flat[flat.index("Not offered:"):]
    for missing in ("locale or caseless order", "several columns in one call", "sort -u", "sre_hip_tally_top_lines",
                    "skips passes by looking at histograms", "Thompson and COUNT scanners", "stream sets"):
        assert missing in own, missing
    for stated in ("exactly those of sre_hip_sort_lines", "a proper prefix first", '"a" < "a\\0" < "a\\0\\0" < "aa"',
                   "stay in line order in BOTH directions", "a second call", "2^32 - 1", "6 sre_int_t", "SIZE_MAX and 0",
                   "chunks of 7 bytes", "LINEAR IN maxlen", "max_bytes is the caller's bound", "exactly as often as in sre_hip_sort_lines",
                   "9 bytes", "24 bytes", "16 bytes", "info untouched"):
        assert stated in flat, stated


def test_the_numeric_sort_is_what_it_was():
    text = header()
    mine = text[text.index("Line sort: the lines of d_buf"):text.index("SRE_API int sre_hip_sort_lines(")]
    flat = " ".join(mine.replace("*", " ").split())
    assert "text or locale order" in flat[flat.index("Not offered:"):] and "sre_hip_sort_lines_text" in flat
    lib = S.load_library()
    sc, side = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(256)
    text = ctypes.create_string_buffer(b"v=1\nv=2\n")
    info = S.SortInfoStruct(*([77] * 10))
    for flags in (8, S.HIP_SORT_DESC | 8, S.HIP_LINES_ALL | 8):
        assert lib.sre_hip_sort_lines(ctypes.addressof(sc), ctypes.addressof(text), 8, 10, 1, flags, 0, ctypes.addressof(side), 64, None, 0,
                                      ctypes.byref(info), None) == -1
    assert [getattr(info, f) for f in S.SortInfo._fields] == [77] * 10


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(S.LIB_PATH)
    assert hasattr(lib, NAME) and hasattr(lib, "sre_hip_sort_text_plan")
    assert NAME in S.API and len(S.API[NAME][1]) == 14 and S.API[NAME][0] is ctypes.c_int
    assert S.SortTextInfo._fields == FIELDS
    assert ctypes.sizeof(S.SortTextInfoStruct) == 9 * ctypes.sizeof(ctypes.c_size_t)


def test_the_mirror_has_the_call():
    sig = inspect.signature(S.Scanner.sort_lines_text)
    assert list(sig.parameters) == ["self", "ptr", "length", "out_ptr", "out_cap", "group", "delim", "max_bytes", "descending",
                                    "all_lines", "limit", "index_ptr", "index_cap", "hip_stream"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"delim": 0x0A, "max_bytes": 0, "descending": False, "all_lines": False, "limit": 0, "index_ptr": None,
                 "index_cap": 0, "hip_stream": None}


def test_the_plan_on_the_host():
    size_max = ctypes.c_size_t(-1).value
    for ln in (0, 1, 6, 7, 8, 14, 15):
        assert len(S.sort_text_plan(ln, ln)) == ln
    assert S.sort_text_plan(0, 0) == [] and S.sort_text_plan(size_max, 0, True) == []
    assert S.sort_text_plan(0, 0, True) == [(0, d) for d in range(8)]
    assert S.sort_text_plan(3, 9) == [(1, 0), (1, 6), (1, 7)] + [(0, d) for d in range(8)]
    assert S.sort_text_plan(7, 9) == [(1, 0), (1, 6), (1, 7)] + [(0, d) for d in range(1, 8)]
    assert S.sort_text_plan(0, 16, True)[:3] == [(2, 0), (2, 6), (2, 7)] and len(S.sort_text_plan(0, 16, True)) == 19
    # a short array receives the front of the list, the length comes back whole
    pairs = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
    assert S.load_library().sre_hip_sort_text_plan(8, 8, 0, pairs, 1) == 8 and list(pairs) == [1, 7, 9, 9]


def test_refusals_that_need_no_device():
    """Every one of these is refused in front of the first look at the scanner or the device: sc stands for an object here and
    is zeroed host memory that a call which got further would trip over."""
    lib = S.load_library()
    sc = ctypes.create_string_buffer(4096)
    text = ctypes.create_string_buffer(b"k=b\nk=a\n")        # (never read)
    side = ctypes.create_string_buffer(256)
    info = S.SortTextInfoStruct(*([77] * 9))
    ok = dict(sc=ctypes.addressof(sc), buf=ctypes.addressof(text), delim=10, group=1, max_bytes=0, flags=0, limit=0,
              out=(ctypes.addressof(side), 64), index=(None, 0))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sre_hip_sort_lines_text(a["sc"], a["buf"], 8, a["delim"], a["group"], a["max_bytes"], a["flags"], a["limit"],
                                           a["out"][0], a["out"][1], a["index"][0], a["index"][1], ctypes.byref(info), None)
    for flags in (S.HIP_LINES_INVERT, S.HIP_LINES_INVERT | S.HIP_LINES_ALL, 8, 1 << 30, S.HIP_SORT_DESC | 8,
                  S.HIP_SORT_DESC | S.HIP_LINES_INVERT):
        assert call(flags=flags) == -1, flags
        assert call(flags=flags, max_bytes=5) == -1, flags
    for name in ("out", "index"):
        assert call(**{name: (None, 3)}) == -1, name
    for delim in (-1, 256, 1000):
        assert call(delim=delim) == -1, delim
    assert call(sc=None) == -1 and call(buf=None) == -1
    assert call(sc=None, flags=S.HIP_SORT_DESC | S.HIP_LINES_ALL, limit=5, max_bytes=3) == -1
    assert call(out=(ctypes.addressof(text) + 2, 4)) == -1          # the output overlaps the buffer
    assert call(sc=None, buf=None, out=(None, 3)) == -1
    assert [getattr(info, f) for f in FIELDS] == [77] * 9
