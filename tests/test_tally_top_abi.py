"""The ordered tally (sre_hip_tally_top_lines): the header declares the enum, the struct and the entry point at the stated
place, libsregex.so exports it, the Python mirror has it, and the argument checks that need no device refuse what the header
says.  No GPU needed."""
import ctypes
import inspect
import os
import re

import sregex_amd as S
import harness

NAME = "sre_hip_tally_top_lines"
FIELDS = ("nlines", "nselected", "nkeys", "nordered", "nrows", "need_bytes", "nwritten", "out_bytes", "passes", "vmin", "vmax")


def header():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        return f.read()


def test_header_declares_the_enum_the_struct_and_the_entry_point():
    text = header()
    assert re.search(r"enum \{ SRE_HIP_TOP_COUNT = 0, SRE_HIP_TOP_SUM = 1, SRE_HIP_TOP_MIN = 2, SRE_HIP_TOP_MAX = 3, "
                     r"SRE_HIP_TOP_N = 4 \};", text)
    assert re.search(r"typedef struct \{\s*size_t\s+nlines;[^}]*size_t\s+nselected;[^}]*size_t\s+nkeys;[^}]*size_t\s+nordered;[^}]*"
                     r"size_t\s+nrows;[^}]*size_t\s+need_bytes, nwritten, out_bytes;[^}]*size_t\s+passes;[^}]*"
                     r"int64_t\s+vmin, vmax;[^}]*\} sre_hip_tally_top_info_t;", text)
    assert re.search(r"int sre_hip_tally_top_lines\(sre_hip_scanner_t \*sc, const void \*d_buf, size_t len, int delim,\s*"
                     r"const int \*groups, size_t ngroups, const int \*vgroups, size_t nvgroups, int fsep, int flags,\s*"
                     r"size_t max_keys, int by, size_t by_col, size_t limit,\s*void \*d_out, size_t out_cap,\s*"
                     r"uint64_t \*d_counts, size_t counts_cap,\s*sre_hip_tally_sum_t \*d_sums, size_t sums_cap,\s*"
                     r"sre_int_t \*d_rank, size_t rank_cap,\s*sre_int_t \*d_index, size_t index_cap,\s*"
                     r"sre_hip_tally_top_info_t \*info, void \*hip_stream\);", text)
    # the block stands behind the line sort's and in front of the stream sets
    assert text.index("SRE_API int sre_hip_sort_lines") < text.index("SRE_HIP_TOP_COUNT") < text.index(
        "SRE_API int sre_hip_tally_top_lines") < text.index("stream sets: many")


def test_the_not_offered_list_and_the_rules_the_header_states():
    text = header()
    mine = text[text.index("Ordered tally: sre_hip_tally_sums_lines whose rows"):text.index("SRE_API int sre_hip_tally_top_lines")]
    flat = " ".join(mine.replace("*", " ").split())
    assert "Not offered:" in flat
    own = flat[flat.index("Not offered:"):]
    for missing in ("order by key text", "several order columns in one call", "a partial top-k selection in place of the full sort",
                    "floating-point averages", "every match of a line", "Thompson and COUNT scanners", "stream sets"):
        assert missing in own, missing
    for stated in ("exactly those of sre_hip_tally_sums_lines", "SRE_HIP_LINES_ALL | SRE_HIP_SORT_DESC", "in BOTH directions",
                   "2^64 - 3", "one diagnostic line", "max_keys <= 2^30", "6 + 2 ngroups", "sre_hip_keyset_create", "FULL order",
                   "INT64_MAX / INT64_MIN", "the full sort, then the cut", "plus two reads", "neither allocate nor fill"):
        assert stated in flat, stated
    # the tally's and the sort's rules are cited, not restated
    assert "007" not in flat and "19 digits" not in flat
    # the older blocks keep their own lists
    assert "keys ordered by count or text, top-k" in text and "a per-line value array supplied by the caller" in text


def test_library_exports_the_entry_point():
    lib = ctypes.CDLL(S.LIB_PATH)
    assert hasattr(lib, NAME)
    assert NAME in S.API and len(S.API[NAME][1]) == 26 and S.API[NAME][0] is ctypes.c_int
    assert S.TallyTopInfo._fields == FIELDS
    assert (S.HIP_TOP_COUNT, S.HIP_TOP_SUM, S.HIP_TOP_MIN, S.HIP_TOP_MAX, S.HIP_TOP_N) == (0, 1, 2, 3, 4)
    assert ctypes.sizeof(S.TallyTopInfoStruct) == 9 * ctypes.sizeof(ctypes.c_size_t) + 16


def test_the_mirror_has_the_call():
    sig = inspect.signature(S.Scanner.tally_top_lines)
    assert list(sig.parameters) == ["self", "ptr", "length", "out_ptr", "out_cap", "groups", "vgroups", "max_keys", "by", "by_col",
                                    "descending", "limit", "delim", "fsep", "all_lines", "counts_ptr", "counts_cap", "sums_ptr",
                                    "sums_cap", "rank_ptr", "rank_cap", "index_ptr", "index_cap", "hip_stream"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"by": S.HIP_TOP_COUNT, "by_col": 0, "descending": True, "limit": 0, "delim": 0x0A, "fsep": 0x09, "all_lines": False,
                 "counts_ptr": None, "counts_cap": 0, "sums_ptr": None, "sums_cap": 0, "rank_ptr": None, "rank_cap": 0,
                 "index_ptr": None, "index_cap": 0, "hip_stream": None}


def test_refusals_that_need_no_device():
    """Every one of these is refused in front of the first look at the scanner or the device: sc stands for an object here and
    is zeroed host memory that a call which got further would trip over."""
    lib = S.load_library()
    sc = ctypes.create_string_buffer(4096)
    text = ctypes.create_string_buffer(b"k=a v=1\nk=b v=2\n")        # (never read)
    side = ctypes.create_string_buffer(512)
    info = S.TallyTopInfoStruct(*([77] * 11))
    groups, vgroups = (ctypes.c_int * 1)(1), (ctypes.c_int * 2)(2, 2)
    at = ctypes.addressof(side)
    ok = dict(sc=ctypes.addressof(sc), buf=ctypes.addressof(text), delim=10, groups=(groups, 1), vgroups=(vgroups, 2), fsep=9, flags=0,
              max_keys=16, by=S.HIP_TOP_SUM, by_col=1, limit=0, out=(at, 64), counts=(at + 64, 2), sums=(at + 128, 2), rank=(at + 256, 2),
              index=(at + 320, 2))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sre_hip_tally_top_lines(a["sc"], a["buf"], 16, a["delim"], a["groups"][0], a["groups"][1], a["vgroups"][0],
                                           a["vgroups"][1], a["fsep"], a["flags"], a["max_keys"], a["by"], a["by_col"], a["limit"],
                                           a["out"][0], a["out"][1], a["counts"][0], a["counts"][1], a["sums"][0], a["sums"][1],
                                           a["rank"][0], a["rank"][1], a["index"][0], a["index"][1], ctypes.byref(info), None)
    for flags in (S.HIP_LINES_INVERT, S.HIP_LINES_INVERT | S.HIP_LINES_ALL, 8, 1 << 30, S.HIP_SORT_DESC | 8,
                  S.HIP_SORT_DESC | S.HIP_LINES_INVERT):
        assert call(flags=flags) == -1, flags
    for by in (-1, 5, 100):
        assert call(by=by) == -1, by
    for by in (S.HIP_TOP_SUM, S.HIP_TOP_MIN, S.HIP_TOP_MAX, S.HIP_TOP_N):
        assert call(by=by, by_col=2) == -1 and call(by=by, by_col=1 << 40) == -1, by
    assert call(by=S.HIP_TOP_COUNT, by_col=1) == -1
    for name in ("out", "counts", "sums", "rank", "index"):
        assert call(**{name: (None, 3)}) == -1, name
    for off in (1, 2, 4, 7):
        assert call(sums=(at + 128 + off, 1)) == -1, off          # d_sums is not 8-byte aligned
    for max_keys in (0, (1 << 30) + 1, 1 << 40):
        assert call(max_keys=max_keys) == -1, max_keys
    # no value groups: only with the count order and no sums
    for by in (S.HIP_TOP_SUM, S.HIP_TOP_MIN, S.HIP_TOP_MAX, S.HIP_TOP_N):
        assert call(vgroups=(None, 0), by=by, by_col=0, sums=(None, 0)) == -1, by
    assert call(vgroups=(None, 0), by=S.HIP_TOP_COUNT, by_col=0) == -1                     # ... sums_cap != 0
    assert call(vgroups=(None, 2)) == -1 and call(vgroups=(vgroups, 0), by=S.HIP_TOP_COUNT, by_col=0, sums=(None, 0)) == -1
    assert call(vgroups=(vgroups, 9)) == -1
    assert call(groups=(None, 1)) == -1 and call(groups=(groups, 0)) == -1 and call(groups=(groups, 33)) == -1
    for fsep in (-1, 256):
        assert call(fsep=fsep) == -1
    for delim in (-1, 256, 1000):
        assert call(delim=delim) == -1, delim
    assert call(sc=None) == -1 and call(buf=None) == -1
    assert call(sc=None, vgroups=(None, 0), by=S.HIP_TOP_COUNT, by_col=0, sums=(None, 0), flags=S.HIP_SORT_DESC | S.HIP_LINES_ALL) == -1
    assert call(out=(ctypes.addressof(text) + 2, 4)) == -1          # the output overlaps the buffer
    assert [getattr(info, f) for f in FIELDS] == [77] * 11
