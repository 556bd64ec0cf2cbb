"""sregex_amd — Python mirror of the sregex C API over the MI355X-native library.

This is a thin ctypes binding of ``sregex_amd/lib/libsregex.so`` (built by
``sregex_amd/csrc/Makefile`` / ``__graft_entry__.build()``).  Names, argument
meaning and error behaviour follow the reference's public header
(reference src/sregex/sregex.h:82-171):

    pool  = Pool()
    re    = parse(pool, [b"a|ab"])            # sre_regex_parse / sre_regex_parse_multi
    prog  = compile(pool, re)                 # sre_regex_compile
    ctx   = PikeCtx(pool, prog, ncaps)        # sre_vm_pike_create_ctx
    rc    = ctx.exec(b"blab", eof=True)       # sre_vm_pike_exec -> rc, ctx.ovector, ctx.pending

plus the additive device-resident batched API of include/sregex_hip.h
(``Scanner``).  The matcher itself runs on the GPU only: with no HIP device the
exec calls return SRE_ERROR and the scanner constructors raise.  Nothing here
imports or calls the test oracle.
"""
import collections
import ctypes
import os
import tempfile

SRE_OK, SRE_ERROR, SRE_AGAIN, SRE_BUSY, SRE_DONE, SRE_DECLINED = 0, -1, -2, -3, -4, -5
SRE_REGEX_CASELESS, SRE_REGEX_NEWLINE = 1, 2
HIP_THOMPSON, HIP_PIKE_FIRST, HIP_PIKE_COUNT = 0, 1, 2
ENGINE_AUTO, ENGINE_VM, ENGINE_SCAN, ENGINE_NFA = 0, 1, 2, 3
HIP_LINES_ALL = 1
HIP_LINES_INVERT = 2
HIP_SORT_DESC = 4
HIP_TOP_COUNT, HIP_TOP_SUM, HIP_TOP_MIN, HIP_TOP_MAX, HIP_TOP_N = 0, 1, 2, 3, 4
HIP_EXTRACT_MAX_FIELDS = 32
HIP_SUBST_MAX_PIECES = 30
HIP_JOIN_MAX_VALUES = 31
HIP_SUBST_MAX_LITERAL = 4096
HIP_ROUTE_MAX_BUCKETS = 256
HIP_TALLY_OVERFLOW = 1
HIP_TALLY_MAX_KEYS = 1 << 30
HIP_TALLY_MAX_VALUES = 8
HIP_DISTINCT_FIRST, HIP_DISTINCT_LAST, HIP_DISTINCT_EVERY = 0, 1, 2
HIP_FOLD_NEXT = 8

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SREGEX_AMD_LIB") or os.path.join(_HERE, "lib", "libsregex.so")

_vp, _sz, _ssz = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_ssize_t
_pssz = ctypes.POINTER(ctypes.c_ssize_t)

# every exported symbol with its signature: (restype, argtypes)
API = {
    # include/sregex/sregex.h
    "sre_create_pool": (_vp, [_sz]),
    "sre_reset_pool": (None, [_vp]),
    "sre_destroy_pool": (None, [_vp]),
    "sre_regex_parse": (_vp, [_vp, ctypes.c_char_p, ctypes.POINTER(_sz), ctypes.c_int, _pssz]),
    "sre_regex_dump": (None, [_vp]),
    "sre_regex_parse_multi": (_vp, [_vp, ctypes.POINTER(ctypes.c_char_p), _ssz, ctypes.POINTER(_sz),
                                    ctypes.POINTER(ctypes.c_int), _pssz, _pssz]),
    "sre_program_dump": (None, [_vp]),
    "sre_regex_compile": (_vp, [_vp, _vp]),
    "sre_vm_pike_create_ctx": (_vp, [_vp, _vp, _pssz, _sz]),
    "sre_vm_pike_exec": (_ssz, [_vp, _vp, _sz, ctypes.c_uint, ctypes.POINTER(_pssz)]),
    "sre_vm_thompson_create_ctx": (_vp, [_vp, _vp]),
    "sre_vm_thompson_exec": (_ssz, [_vp, _vp, _sz, ctypes.c_uint]),
    "sre_vm_thompson_jit_compile": (_ssz, [_vp, _vp, ctypes.POINTER(_vp)]),
    "sre_vm_thompson_jit_create_ctx": (_vp, [_vp, _vp]),
    "sre_vm_thompson_jit_get_handler": (_vp, [_vp]),
    "sre_vm_thompson_jit_free": (_ssz, [_vp]),
    # include/sregex_hip.h
    "sre_hip_device_count": (ctypes.c_int, []),
    "sre_hip_set_device": (ctypes.c_int, [ctypes.c_int]),
    "sre_hip_scanner_create": (_vp, [_vp, _vp, ctypes.c_int, ctypes.c_int]),
    "sre_hip_scanner_engine": (ctypes.c_int, [_vp]),
    "sre_hip_scanner_result_slots": (_sz, [_vp]),
    "sre_hip_scanner_set_segment_bytes": (ctypes.c_int, [_vp, _sz]),
    "sre_hip_scanner_last_fixups": (ctypes.c_int, [_vp]),
    "sre_hip_scanner_last_lineage_passes": (ctypes.c_int, [_vp]),
    "sre_hip_scanner_last_exact_passes": (ctypes.c_int, [_vp]),
    "sre_hip_scanner_last_count_rounds": (ctypes.c_int, [_vp]),
    "sre_hip_compat_route_counts": (None, [ctypes.POINTER(ctypes.c_ulonglong)]),
    "sre_hip_compat_trim": (ctypes.c_int, []),
    "sre_hip_scanner_set_tail_stream": (ctypes.c_int, [_vp, _vp]),
    "sre_hip_scanner_class_bits": (ctypes.c_int, [_vp]),
    "sre_hip_scanner_nfa_bits": (ctypes.c_int, [_vp]),
    "sre_hip_scanner_kernel_name": (ctypes.c_char_p, [_vp]),
    "sre_hip_scanner_last_kernel_ms": (ctypes.c_double, [_vp]),
    "sre_hip_scanner_last_segment_bytes": (_sz, [_vp]),
    "sre_hip_scanner_order_after_scan": (ctypes.c_int, [_vp, _vp]),
    "sre_hip_scan_enqueue": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_sz), _sz, _vp]),
    "sre_hip_scan_results": (ctypes.c_int, [_vp, _pssz]),
    "sre_hip_scan_batch": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_sz), _sz, _pssz, _vp]),
    "sre_hip_scan_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int, _pssz, _sz,
                                          ctypes.POINTER(_sz), ctypes.POINTER(_sz), _vp]),
    "sre_hip_filter_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sre_hip_filter_lines_context": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int, _sz, _sz, _vp, _sz, _vp, _sz, _vp,
                                                    _vp]),
    "sre_hip_fold_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, _sz, _vp, _sz, _vp, _sz, _vp, _sz,
                                          _vp, _vp]),
    "sre_hip_extract_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _sz, ctypes.c_int,
                                             ctypes.c_int, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sre_hip_subst_template_check": (ctypes.c_int, [ctypes.c_char_p, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                    ctypes.POINTER(_sz)]),
    "sre_hip_substitute_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_char_p, _sz, ctypes.c_int, _vp, _sz, _vp, _sz,
                                                _vp, _vp]),
    "sre_hip_route_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _sz, _vp, _sz, _vp, _sz, _vp,
                                           _vp, _vp]),
    "sre_hip_tally_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _sz, ctypes.c_int,
                                           ctypes.c_int, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sre_hip_tally_sums_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _sz,
                                                ctypes.POINTER(ctypes.c_int), _sz, ctypes.c_int, ctypes.c_int, _sz, _vp, _sz, _vp, _sz,
                                                _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sre_hip_tally_number": (ctypes.c_int, [ctypes.c_char_p, _sz, ctypes.POINTER(ctypes.c_int64)]),
    "sre_hip_keyset_create": (_vp, [_vp, _sz, _sz, ctypes.c_int, ctypes.c_int, _vp]),
    "sre_hip_keyset_create_map": (_vp, [_vp, _sz, _sz, _sz, ctypes.c_int, ctypes.c_int, _vp]),
    "sre_hip_keyset_values": (_sz, [_vp]),
    "sre_hip_keyset_destroy": (None, [_vp]),
    "sre_hip_keyset_rows": (_sz, [_vp]),
    "sre_hip_keyset_distinct": (_sz, [_vp]),
    "sre_hip_keyset_fields": (_sz, [_vp]),
    "sre_hip_keyset_slots": (_sz, [_vp]),
    "sre_hip_keyset_device_bytes": (_sz, [_vp]),
    "sre_hip_keyset_hash": (ctypes.c_uint64, [ctypes.c_char_p, _sz, _sz, ctypes.c_int]),
    "sre_hip_lookup_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _sz, _vp, ctypes.c_int, _vp,
                                            _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sre_hip_distinct_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _sz, ctypes.c_int, _sz, _sz,
                                              ctypes.c_int, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sre_hip_join_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _sz, _vp,
                                          ctypes.POINTER(ctypes.c_int), _sz, ctypes.c_int, ctypes.c_int, _vp, _sz, _vp, _sz, _vp, _sz,
                                          _vp, _vp]),
    "sre_hip_route_lines_by_key": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _sz, _vp, ctypes.c_int,
                                                  _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sre_hip_sort_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sre_hip_sort_lines_text": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int, _sz, ctypes.c_int, _sz, _vp, _sz, _vp, _sz, _vp,
                                               _vp]),
    "sre_hip_sort_text_plan": (_sz, [_sz, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), _sz]),
    "sre_hip_tally_top_lines": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _sz,
                                               ctypes.POINTER(ctypes.c_int), _sz, ctypes.c_int, ctypes.c_int, _sz, ctypes.c_int, _sz,
                                               _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sre_hip_scanner_last_line_batches": (ctypes.c_int, [_vp]),
    "sre_hip_scanner_last_lines_device": (ctypes.c_int, [_vp]),
    "sre_hip_scanner_last_short_lines": (_sz, [_vp]),
    "sre_hip_streams_create": (_vp, [_vp, _vp, ctypes.c_int, _sz]),
    "sre_hip_streams_create_engine": (_vp, [_vp, _vp, ctypes.c_int, ctypes.c_int, _sz]),
    "sre_hip_streams_engine": (ctypes.c_int, [_vp]),
    "sre_hip_streams_nfa_bits": (ctypes.c_int, [_vp]),
    "sre_hip_streams_last_exact_passes": (ctypes.c_int, [_vp]),
    "sre_hip_streams_count": (_sz, [_vp]),
    "sre_hip_streams_result_slots": (_sz, [_vp]),
    "sre_hip_streams_device_bytes": (_sz, [_vp]),
    "sre_hip_streams_feed": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_sz),
                                            ctypes.POINTER(ctypes.c_ubyte), _pssz, _vp]),
    "sre_hip_streams_reset": (ctypes.c_int, [_vp, ctypes.POINTER(_sz), _sz]),
    "sre_hip_streams_last_fixups": (ctypes.c_int, [_vp]),
    "sre_hip_streams_last_launches": (ctypes.c_int, [_vp]),
    "sre_hip_alloc": (_vp, [_sz]),
    "sre_hip_free": (None, [_vp]),
    "sre_hip_upload": (ctypes.c_int, [_vp, _vp, _sz]),
    "sre_hip_download": (ctypes.c_int, [_vp, _vp, _sz]),
    "sre_hip_synchronize": (ctypes.c_int, [_vp]),
    "sre_hip_gen_data": (ctypes.c_int, [_vp, _sz, ctypes.c_char_p, _sz, _vp]),
    "sre_hip_read_ceiling": (ctypes.c_int, [_vp, _sz, _vp]),
    "sre_hip_read_pattern": (ctypes.c_int, [_vp, _sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, _vp]),
}

_lib = None
_libc = None


def _missing_symbol(name, path):
    def fail(*_a, **_k):
        raise RuntimeError("%s is not exported by %s (SREGEX_AMD_LIB points at an older build)" % (name, path))
    return fail


def load_library(path=None):
    """Load libsregex.so and declare every entry point.  Fails loudly if the
    library has not been built (see __graft_entry__.build())."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            "%s is missing: build it with `make -C sregex_amd/csrc` "
            "(or __graft_entry__.build()); there is no pure-Python matcher" % p)
    lib = ctypes.CDLL(p)
    for name, (res, args) in API.items():
        if os.environ.get("SREGEX_AMD_LIB") and not hasattr(lib, name):
            # an older build given for an A/B run (tools/exp_knobs.sh) may lack the newest entry points:
            # such a name fails on first USE with a clear message, never with ctypes' default int restype
            setattr(lib, name, _missing_symbol(name, p))
            continue
        fn = getattr(lib, name)      # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def template_pieces(template, max_group):
    """sre_hip_subst_template_check: the pieces of a substitute template (Scanner.substitute_lines) as a list, the
    capture group number of each piece or -1 for a literal piece; max_group is the largest group the template may
    name (a scanner's (slots - 2) // 2 - 1).  Raises ValueError for an invalid template.  Needs no device."""
    template = bytes(template)
    groups = (ctypes.c_int * HIP_SUBST_MAX_PIECES)()
    n = _sz()
    if load_library().sre_hip_subst_template_check(template, len(template), max_group, groups, ctypes.byref(n)) != 0:
        raise ValueError("invalid substitute template %r for max_group %d" % (template, max_group))
    return list(groups[:n.value])


def tally_number(text):
    """sre_hip_tally_number: the value of `text` (bytes) under the number rule of Scanner.tally_sums_lines (an optional
    '-' and 1 to 18 decimal digits, nothing else) as an int, or None when it is not a number.  Needs no device."""
    text = bytes(text)
    value = ctypes.c_int64()
    if load_library().sre_hip_tally_number(text, len(text), ctypes.byref(value)) != 1:
        return None
    return value.value


def sort_text_plan(minlen, maxlen, rest=False):
    """sre_hip_sort_text_plan: the digit passes of Scanner.sort_lines_text as a list of (chunk, digit) in the order they
    run, from the minlen and maxlen its info reports and rest (all_lines with at least one line without a match); digit 0
    is a chunk's count byte, digit 7 - j its byte j.  SortTextInfo.passes is its length.  Needs no device."""
    lib = load_library()
    n = lib.sre_hip_sort_text_plan(minlen, maxlen, int(bool(rest)), None, 0)
    pairs = (ctypes.c_uint64 * (2 * max(n, 1)))()
    if lib.sre_hip_sort_text_plan(minlen, maxlen, int(bool(rest)), pairs, n) != n:
        raise RuntimeError("sre_hip_sort_text_plan failed")
    return [(pairs[2 * i], pairs[2 * i + 1]) for i in range(n)]


def keyset_hash(row, nfields=1, fsep=0x09):
    """sre_hip_keyset_hash: the hash a KeySet of nfields fields gives the row `row` (bytes, without its delimiter); the
    row's home slot in a set is keyset_hash(row) & (set.slots - 1).  0 for a row that does not hold nfields fields.
    Needs no device."""
    row = bytes(row)
    return load_library().sre_hip_keyset_hash(row, len(row), nfields, fsep)


class KeySet:
    """sre_hip_keyset_*: the distinct keys of a dictionary of rows (field 0, fsep, .., field K - 1, delim: what
    Scanner.extract_lines and Scanner.tally_lines write) in the device buffer (ptr, length), kept on the device for
    Scanner.lookup_lines.  The set copies the rows: the buffer may be freed once the constructor has returned.  A key's
    id is the lowest row that carries it.  With nkeys (sre_hip_keyset_create_map) the set is a key MAP: the first nkeys
    of a row's nfields fields are its key, the others the value columns Scanner.join_lines appends to a line; the values
    of a key are those of the lowest row that carries it.  Raises ValueError when the arguments are out of range or a
    row does not hold nfields fields."""

    def __init__(self, ptr, length, nfields=1, fsep=0x09, delim=0x0A, hip_stream=None, lib=None, nkeys=None):
        self.lib = lib or load_library()
        if nkeys is None:
            self.h = self.lib.sre_hip_keyset_create(ptr, length, nfields, fsep, delim, hip_stream)
        else:
            self.h = self.lib.sre_hip_keyset_create_map(ptr, length, nfields, nkeys, fsep, delim, hip_stream)
        if not self.h:
            raise ValueError("sre_hip_keyset_create%s failed (arguments out of range, a row without %d fields, or no device)"
                             % ("" if nkeys is None else "_map", nfields))

    def close(self):
        if self.h:
            self.lib.sre_hip_keyset_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def rows(self):
        return self.lib.sre_hip_keyset_rows(self.h)

    @property
    def distinct(self):
        return self.lib.sre_hip_keyset_distinct(self.h)

    @property
    def fields(self):
        return self.lib.sre_hip_keyset_fields(self.h)

    @property
    def values(self):
        """value columns of a key map; 0 for a plain set"""
        return self.lib.sre_hip_keyset_values(self.h)

    @property
    def slots(self):
        return self.lib.sre_hip_keyset_slots(self.h)

    @property
    def device_bytes(self):
        return self.lib.sre_hip_keyset_device_bytes(self.h)


def _capture_stdout(fn):
    """Run fn() and return what C stdio wrote to fd 1 (the dumps use printf)."""
    global _libc
    if _libc is None:
        _libc = ctypes.CDLL(None)
    _libc.fflush(None)
    with tempfile.TemporaryFile() as tf:
        saved = os.dup(1)
        os.dup2(tf.fileno(), 1)
        try:
            fn()
            _libc.fflush(None)
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        tf.seek(0)
        return tf.read()


class SyntaxError_(Exception):
    """Regex syntax error; str() is the reference CLI's message
    (reference src/sre_cli.c:121, 156)."""

    def __init__(self, offset, regex_id=None):
        self.offset, self.regex_id = offset, regex_id
        if regex_id is None:
            msg = "[error] syntax error at pos %d" % offset
        else:
            msg = "[error] regex %d: syntax error at pos %d" % (regex_id, offset)
        super().__init__(msg)


class Pool:
    def __init__(self, size=1024):
        self.lib = load_library()
        self.p = self.lib.sre_create_pool(size)
        if not self.p:
            raise MemoryError("sre_create_pool")

    def reset(self):
        self.lib.sre_reset_pool(self.p)

    def destroy(self):
        if self.p:
            self.lib.sre_destroy_pool(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.destroy()


class Regex:
    def __init__(self, pool, handle, ncaps, nregexes):
        self.pool, self.h, self.ncaps, self.nregexes = pool, handle, ncaps, nregexes

    def dump(self):
        lib = self.pool.lib
        return _capture_stdout(lambda: lib.sre_regex_dump(self.h)).decode("latin-1")


def parse(pool, regexes, flags=None, multi=None):
    """sre_regex_parse for one regex, sre_regex_parse_multi for several (or when
    multi=True).  `flags` is a list of per-regex flag ints.  Raises SyntaxError_."""
    lib = pool.lib
    regexes = [bytes(r).split(b"\0")[0] for r in regexes]   # C strings
    if multi is None:
        multi = len(regexes) != 1
    ncaps = _sz(0)
    eo = _ssz(-1)
    if not multi:
        h = lib.sre_regex_parse(pool.p, regexes[0], ctypes.byref(ncaps),
                                (flags or [0])[0], ctypes.byref(eo))
        if not h:
            raise SyntaxError_(eo.value)
    else:
        arr = (ctypes.c_char_p * len(regexes))(*regexes)
        fl = (ctypes.c_int * len(regexes))(*flags) if flags else None
        ei = _ssz(-1)
        h = lib.sre_regex_parse_multi(pool.p, arr, len(regexes), ctypes.byref(ncaps), fl,
                                      ctypes.byref(eo), ctypes.byref(ei))
        if not h:
            raise SyntaxError_(eo.value, ei.value)
    return Regex(pool, h, ncaps.value, len(regexes))


class Program:
    def __init__(self, pool, handle, ncaps, nregexes):
        self.pool, self.h, self.ncaps, self.nregexes = pool, handle, ncaps, nregexes

    def dump(self):
        lib = self.pool.lib
        return _capture_stdout(lambda: lib.sre_program_dump(self.h)).decode("latin-1")


def compile(pool, regex):
    h = pool.lib.sre_regex_compile(pool.p, regex.h)
    if not h:
        raise RuntimeError("sre_regex_compile failed")
    return Program(pool, h, regex.ncaps, regex.nregexes)


def _as_buffer(data):
    """bytes -> (pointer or None, length); NULL for empty input like the CLI's
    splitted modes (reference src/sre_cli.c:373-376)."""
    if data is None or len(data) == 0:
        return None, 0, None
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    return ctypes.cast(buf, _vp), len(data), buf


class PikeCtx:
    """sre_vm_pike_create_ctx / sre_vm_pike_exec.  `ovector` is caller-owned and
    sized 2 * (ncaps + 1), as the reference clients do (src/sre_cli.c:204-205)."""

    def __init__(self, pool, prog, ncaps=None):
        self.lib = pool.lib
        n = 2 * ((prog.ncaps if ncaps is None else ncaps) + 1)
        self.nov = n
        self.ovector = (ctypes.c_ssize_t * n)(*([0] * n))
        self.h = self.lib.sre_vm_pike_create_ctx(pool.p, prog.h, self.ovector, n * 8)
        if not self.h:
            raise MemoryError("sre_vm_pike_create_ctx")
        self.pending = None

    def exec(self, data, eof, want_pending=True, base=None, offset=0, length=None):
        """Feed one chunk.  With `base` (a ctypes buffer) the chunk is
        base[offset:offset+length] — lets a caller re-feed from a match end
        without copying (find-all iteration)."""
        if base is not None:
            ptr = ctypes.cast(ctypes.addressof(base) + offset, _vp)
            n = length
            keep = base
        else:
            ptr, n, keep = _as_buffer(data)
        pend = _pssz()
        rc = self.lib.sre_vm_pike_exec(self.h, ptr, n, 1 if eof else 0,
                                       ctypes.byref(pend) if want_pending else None)
        self.pending = (pend[0], pend[1]) if (want_pending and rc == SRE_AGAIN and pend) else None
        del keep
        return rc


class ThompsonCtx:
    """sre_vm_thompson_create_ctx / sre_vm_thompson_exec."""

    def __init__(self, pool, prog):
        self.lib = pool.lib
        self.h = self.lib.sre_vm_thompson_create_ctx(pool.p, prog.h)
        if not self.h:
            raise MemoryError("sre_vm_thompson_create_ctx")

    def exec(self, data, eof):
        ptr, n, keep = _as_buffer(data)
        rc = self.lib.sre_vm_thompson_exec(self.h, ptr, n, 1 if eof else 0)
        del keep
        return rc


class Scanner:
    """sre_hip_scanner_create + scan_* (include/sregex_hip.h): many device-resident
    streams, one compiled program."""

    def __init__(self, pool, prog, mode, engine=ENGINE_AUTO):
        self.lib = pool.lib
        self.h = self.lib.sre_hip_scanner_create(pool.p, prog.h, mode, engine)
        if not self.h:
            raise RuntimeError("sre_hip_scanner_create failed (no HIP device, or the requested "
                               "engine does not take this program)")
        self.slots = self.lib.sre_hip_scanner_result_slots(self.h)
        self.engine = self.lib.sre_hip_scanner_engine(self.h)
        self.nregexes = prog.nregexes
        self._n = 0

    def set_segment_bytes(self, nbytes):
        if self.lib.sre_hip_scanner_set_segment_bytes(self.h, nbytes) != 0:
            raise ValueError("segment size must be a multiple of 64")

    @property
    def engine_name(self):
        return {ENGINE_VM: "vm", ENGINE_SCAN: "scan", ENGINE_NFA: "nfa"}.get(self.engine, "?")

    @property
    def kernel_name(self):
        """the dominant kernel of a scan, as rocprofv3 names it"""
        return self.lib.sre_hip_scanner_kernel_name(self.h).decode()

    @property
    def last_exact_passes(self):
        return self.lib.sre_hip_scanner_last_exact_passes(self.h)

    @property
    def last_count_rounds(self):
        return self.lib.sre_hip_scanner_last_count_rounds(self.h)

    @property
    def last_lineage_passes(self):
        return self.lib.sre_hip_scanner_last_lineage_passes(self.h)

    @property
    def class_bits(self):
        return self.lib.sre_hip_scanner_class_bits(self.h)

    @property
    def nfa_bits(self):
        """bits of a lane's thread set on the NFA tier (64, 128 or 256), 0 on the other engines"""
        return self.lib.sre_hip_scanner_nfa_bits(self.h)

    @property
    def last_kernel_ms(self):
        return self.lib.sre_hip_scanner_last_kernel_ms(self.h)

    @property
    def last_segment_bytes(self):
        return self.lib.sre_hip_scanner_last_segment_bytes(self.h)

    @property
    def last_fixups(self):
        return self.lib.sre_hip_scanner_last_fixups(self.h)

    def set_tail_stream(self, hip_stream):
        """queue what follows the scan kernel of every later call on hip_stream (see sregex_hip.h)"""
        if self.lib.sre_hip_scanner_set_tail_stream(self.h, hip_stream) != 0:
            raise RuntimeError("sre_hip_scanner_set_tail_stream failed")

    def order_after_scan(self, hip_stream):
        """make hip_stream wait for this scanner's last scan kernel (see sregex_hip.h)"""
        if self.lib.sre_hip_scanner_order_after_scan(self.h, hip_stream) != 0:
            raise RuntimeError("sre_hip_scanner_order_after_scan failed")

    def enqueue(self, d_ptrs, lens, hip_stream=None):
        n = len(d_ptrs)
        a = (_vp * n)(*d_ptrs)
        b = (_sz * n)(*lens)
        self._n = n
        if self.lib.sre_hip_scan_enqueue(self.h, a, b, n, hip_stream) != 0:
            raise RuntimeError("sre_hip_scan_enqueue failed")

    def results(self):
        out = (ctypes.c_ssize_t * (self._n * self.slots))()
        if self.lib.sre_hip_scan_results(self.h, out) != 0:
            raise RuntimeError("sre_hip_scan_results failed")
        s = self.slots
        return [list(out[i * s:(i + 1) * s]) for i in range(self._n)]

    def scan(self, d_ptrs, lens, hip_stream=None):
        self.enqueue(d_ptrs, lens, hip_stream)
        return self.results()

    def scan_lines(self, ptr, length, delim=0x0A, all_lines=False, cap=1 << 20, hip_stream=None):
        """sre_hip_scan_lines: every line of the device buffer (ptr, length) as its own stream.
        Returns (nlines, nreported, rows); a row is [line no, start, length] + the line's record,
        and rows holds the first min(cap, nreported) reported lines in order."""
        width = 3 + self.slots
        out = (ctypes.c_ssize_t * (cap * width))() if cap else None
        nl, nr = _sz(), _sz()
        if self.lib.sre_hip_scan_lines(self.h, ptr, length, delim, HIP_LINES_ALL if all_lines else 0, out, cap,
                                       ctypes.byref(nl), ctypes.byref(nr), hip_stream) != 0:
            raise RuntimeError("sre_hip_scan_lines failed")
        take = min(cap, nr.value)
        rows = [list(out[i * width:(i + 1) * width]) for i in range(take)]
        return nl.value, nr.value, rows

    def filter_lines(self, ptr, length, out_ptr, out_cap, delim=0x0A, invert=False, all_lines=False, index_ptr=None,
                     index_cap=0, hip_stream=None):
        """sre_hip_filter_lines: the selected lines of the device buffer (ptr, length), each followed by one
        delimiter, compacted in order into the device buffer (out_ptr, out_cap); index_ptr: an optional device
        array of index_cap rows [line no, offset in the buffer, length, offset in the output].  Returns
        FilterInfo(nlines, nselected, need_bytes, nwritten, out_bytes)."""
        flags = (HIP_LINES_ALL if all_lines else 0) | (HIP_LINES_INVERT if invert else 0)
        info = (_sz * 5)()
        if self.lib.sre_hip_filter_lines(self.h, ptr, length, delim, flags, out_ptr, out_cap, index_ptr, index_cap,
                                         info, hip_stream) != 0:
            raise RuntimeError("sre_hip_filter_lines failed")
        return FilterInfo(*info)

    def filter_lines_context(self, ptr, length, out_ptr, out_cap, before=0, after=0, delim=0x0A, invert=False, index_ptr=None,
                             index_cap=0, hip_stream=None):
        """sre_hip_filter_lines_context: filter_lines with context lines (grep -B before -A after): the matching lines
        of the device buffer (ptr, length), with invert the lines without a match, and every line at most `before`
        lines in front of one or `after` lines behind one, each once, in line order, each followed by one delimiter,
        in the device buffer (out_ptr, out_cap).  index_ptr: an optional device array of index_cap rows of FIVE words
        [line no, offset in the buffer, length, offset in the output, flags]; flags bit 0: a context-only line, bit 1:
        the first line of a group of adjacent selected lines.  Returns ContextInfo(nlines, nmatched, nselected,
        ngroups, need_bytes, nwritten, out_bytes)."""
        info = (_sz * 7)()
        if self.lib.sre_hip_filter_lines_context(self.h, ptr, length, delim, HIP_LINES_INVERT if invert else 0, before, after,
                                                 out_ptr, out_cap, index_ptr, index_cap, info, hip_stream) != 0:
            raise RuntimeError("sre_hip_filter_lines_context failed")
        return ContextInfo(*info)

    def fold_lines(self, ptr, length, out_ptr, out_cap, join=0x01, max_lines=0, delim=0x0A, invert=False, fold_next=False,
                   recid_ptr=None, recid_cap=0, records_ptr=None, records_cap=0, hip_stream=None):
        """sre_hip_fold_lines: the lines of the device buffer (ptr, length) joined into multi-line records in the device
        buffer (out_ptr, out_cap): every line is written in line order, followed by the delimiter when it is the last of
        its record and by the byte `join` otherwise.  A line with a match (with invert: without one) is MARKED: it
        belongs to the record of the line in front of it, with fold_next it continues into the line behind it;
        max_lines caps the lines of a record (0: no cap).  Only whole records are written.  recid_ptr: an optional
        device array of recid_cap words, the record number of each line; records_ptr: an optional device array of
        records_cap rows [first line, lines, offset in the buffer, bytes in the output without the final delimiter,
        offset in the output].  Returns FoldInfo(nlines, nmarked, nrecords, longest, need_bytes, nwritten, out_bytes)."""
        if (not 0 <= join <= 255 or max_lines < 0 or (recid_ptr is None) != (recid_cap == 0)
                or (records_ptr is None) != (records_cap == 0) or (out_ptr is None and out_cap != 0)):
            raise ValueError("sre_hip_fold_lines: join outside 0..255, or a pointer that does not stand for its capacity")
        flags = (HIP_LINES_INVERT if invert else 0) | (HIP_FOLD_NEXT if fold_next else 0)
        info = FoldInfoStruct()
        if self.lib.sre_hip_fold_lines(self.h, ptr, length, delim, flags, join, max_lines, out_ptr, out_cap, recid_ptr, recid_cap,
                                       records_ptr, records_cap, ctypes.byref(info), hip_stream) != 0:
            raise RuntimeError("sre_hip_fold_lines failed")
        return FoldInfo(*(getattr(info, name) for name in FoldInfo._fields))

    def extract_lines(self, ptr, length, groups, out_ptr, out_cap, delim=0x0A, fsep=0x09, all_lines=False, index_ptr=None,
                      index_cap=0, hip_stream=None):
        """sre_hip_extract_lines: for every matching line of the device buffer (ptr, length) (every line with
        all_lines) one row in the device buffer (out_ptr, out_cap): the text of the capture groups `groups` of the
        line's first match, separated by fsep and ended by delim; an unset group is an empty field.  index_ptr: an
        optional device array of index_cap rows [line no, offset in the buffer, length, offset of the row in the
        output] + [offset in the buffer, length] per field ([-1, -1]: unset).  The scanner's mode must be
        HIP_PIKE_FIRST.  Returns FilterInfo(nlines, nselected, need_bytes, nwritten, out_bytes), counts of lines."""
        groups = list(groups)
        arr = (ctypes.c_int * max(len(groups), 1))(*groups)
        info = (_sz * 5)()
        if self.lib.sre_hip_extract_lines(self.h, ptr, length, delim, arr, len(groups), fsep, HIP_LINES_ALL if all_lines else 0,
                                          out_ptr, out_cap, index_ptr, index_cap, info, hip_stream) != 0:
            raise RuntimeError("sre_hip_extract_lines failed")
        return FilterInfo(*info)

    def substitute_lines(self, ptr, length, template, out_ptr, out_cap, delim=0x0A, all_lines=False, index_ptr=None,
                         index_cap=0, hip_stream=None):
        """sre_hip_substitute_lines: for every matching line of the device buffer (ptr, length) one row in the device
        buffer (out_ptr, out_cap): the line with its FIRST match replaced by `template` (host bytes: $1 / ${1} a
        capture group, $$ a dollar, anything else literal), ended by delim; with all_lines every line, a line
        without a match copied unchanged.  index_ptr: an optional device array of index_cap rows [line no, offset in
        the buffer, length, offset of the row in the output, offset in the buffer and length of the match, offset in
        the output and length of the replacement] (the last four -1 for an unmatched line).  The scanner's mode must
        be HIP_PIKE_FIRST.  Returns FilterInfo(nlines, nselected, need_bytes, nwritten, out_bytes), counts of lines."""
        template = bytes(template)
        info = (_sz * 5)()
        if self.lib.sre_hip_substitute_lines(self.h, ptr, length, delim, template, len(template),
                                             HIP_LINES_ALL if all_lines else 0, out_ptr, out_cap, index_ptr, index_cap, info,
                                             hip_stream) != 0:
            raise RuntimeError("sre_hip_substitute_lines failed")
        return FilterInfo(*info)

    def route_lines(self, ptr, length, out_ptr, out_cap, bucket_of=None, nbuckets=None, delim=0x0A, index_ptr=None,
                    index_cap=0, hip_stream=None):
        """sre_hip_route_lines: every line of the device buffer (ptr, length) goes to the bucket of the regex of its
        first match: bucket_of[r] for regex r, bucket_of[nregexes] for a line without a match, -1 drops the line; None is
        the identity with unmatched lines dropped (nbuckets then defaults to the program's regexes).  The device buffer
        (out_ptr, out_cap) receives all lines of bucket 0 in line order, then bucket 1, .., each followed by one
        delimiter.  index_ptr: an optional device array of index_cap rows [line no, offset in the buffer, length, offset
        in the output, bucket] in output order.  The scanner's mode must be HIP_PIKE_FIRST.  Returns (FilterInfo(nlines,
        nselected, need_bytes, nwritten, out_bytes), [RouteBucket(nlines, offset, bytes)] per bucket): the buckets'
        totals over the whole buffer whatever out_cap is, offset where the bucket starts when everything fits."""
        arr = None
        if bucket_of is not None:
            bucket_of = list(bucket_of)
            if len(bucket_of) != self.nregexes + 1:
                raise ValueError("bucket_of needs nregexes + 1 = %d entries" % (self.nregexes + 1))
            arr = (ctypes.c_int * len(bucket_of))(*bucket_of)
            if nbuckets is None:
                nbuckets = max(bucket_of) + 1
        elif nbuckets is None:
            nbuckets = self.nregexes
        info = (_sz * 5)()
        bk = (_sz * (3 * max(nbuckets, 1)))()
        if self.lib.sre_hip_route_lines(self.h, ptr, length, delim, arr, nbuckets, out_ptr, out_cap, index_ptr, index_cap, info,
                                        bk, hip_stream) != 0:
            raise RuntimeError("sre_hip_route_lines failed")
        return FilterInfo(*info), [RouteBucket(*bk[3 * b:3 * b + 3]) for b in range(nbuckets)]

    def tally_lines(self, ptr, length, out_ptr, out_cap, groups, max_keys, delim=0x0A, fsep=0x09, flags=0, counts_ptr=None,
                    counts_cap=0, keyid_ptr=None, keyid_cap=0, index_ptr=None, index_cap=0, hip_stream=None):
        """sre_hip_tally_lines: the distinct keys of the device buffer (ptr, length) and how many lines carry each.  The
        key of a matching line (of every line with flags=HIP_LINES_ALL) is the tuple of the texts of the capture groups
        `groups` of its first match, as extract_lines defines them.  The device buffer (out_ptr, out_cap) receives one
        row per distinct key in the extract's row format, ordered by the first line that carries each key: row k is the
        row extract_lines writes for that line.  counts_ptr: an optional device array of counts_cap uint64, the lines
        of key k; keyid_ptr: an optional device array of keyid_cap int64, the key number of line i or -1; index_ptr: an
        optional device array of index_cap of the extract's index rows, each describing a key's first line.  Counts and
        key ids are complete whatever out_cap is.  The scanner's mode must be HIP_PIKE_FIRST.  Returns
        TallyInfo(nlines, nselected, nkeys, need_bytes, nwritten, out_bytes).  More than max_keys distinct keys raise
        TallyOverflow, whose .info holds nlines and nselected and zeros elsewhere; nothing was written then."""
        groups = list(groups)
        arr = (ctypes.c_int * max(len(groups), 1))(*groups)
        info = TallyInfoStruct()
        rc = self.lib.sre_hip_tally_lines(self.h, ptr, length, delim, arr, len(groups), fsep, flags, max_keys, out_ptr, out_cap,
                                          counts_ptr, counts_cap, keyid_ptr, keyid_cap, index_ptr, index_cap, ctypes.byref(info),
                                          hip_stream)
        res = TallyInfo(info.nlines, info.nselected, info.nkeys, info.need_bytes, info.nwritten, info.out_bytes)
        if rc == HIP_TALLY_OVERFLOW:
            raise TallyOverflow(res, max_keys)
        if rc != 0:
            raise RuntimeError("sre_hip_tally_lines failed")
        return res

    def tally_sums_lines(self, ptr, length, out_ptr, out_cap, groups, vgroups, max_keys, delim=0x0A, fsep=0x09, flags=0,
                         counts_ptr=None, counts_cap=0, sums_ptr=None, sums_cap=0, keyid_ptr=None, keyid_cap=0, index_ptr=None,
                         index_cap=0, hip_stream=None):
        """sre_hip_tally_sums_lines: tally_lines with the same arguments and results, and per key the sum, minimum,
        maximum and count of the numbers in the capture groups `vgroups` (1 .. HIP_TALLY_MAX_VALUES of them) of the
        key's lines.  sums_ptr: an optional device array of sums_cap rows of len(vgroups) TallySumStruct, row k the
        aggregates of key k; a text is a number when tally_number() says so, anything else touches nothing, and a
        column without a number is (0, INT64_MAX, INT64_MIN, 0).  The sum wraps modulo 2^64.  Returns TallyInfo; raises
        TallyOverflow as tally_lines does, with nothing written."""
        groups, vgroups = list(groups), list(vgroups)
        arr = (ctypes.c_int * max(len(groups), 1))(*groups)
        varr = (ctypes.c_int * max(len(vgroups), 1))(*vgroups)
        info = TallyInfoStruct()
        rc = self.lib.sre_hip_tally_sums_lines(self.h, ptr, length, delim, arr, len(groups), varr, len(vgroups), fsep, flags,
                                               max_keys, out_ptr, out_cap, counts_ptr, counts_cap, sums_ptr, sums_cap, keyid_ptr,
                                               keyid_cap, index_ptr, index_cap, ctypes.byref(info), hip_stream)
        res = TallyInfo(info.nlines, info.nselected, info.nkeys, info.need_bytes, info.nwritten, info.out_bytes)
        if rc == HIP_TALLY_OVERFLOW:
            raise TallyOverflow(res, max_keys)
        if rc != 0:
            raise RuntimeError("sre_hip_tally_sums_lines failed")
        return res

    def lookup_lines(self, ptr, length, out_ptr, out_cap, groups, keyset, delim=0x0A, invert=False, keyid_ptr=None, keyid_cap=0,
                     index_ptr=None, index_cap=0, hip_stream=None):
        """sre_hip_lookup_lines: the matching lines of the device buffer (ptr, length) whose key, the tuple of the texts of
        the capture groups `groups` of the first match, is in the KeySet `keyset` (with invert: is not in it), each
        followed by one delimiter, compacted in order into the device buffer (out_ptr, out_cap) as filter_lines writes
        them.  keyid_ptr: an optional device array of keyid_cap int64, per line the id of its key in the set (a row of the
        dictionary), -1 for a key the set does not hold, -2 for a line without a match; index_ptr: the filter's index
        rows.  The scanner's mode must be HIP_PIKE_FIRST.  Returns LookupInfo(nlines, nkeyed, nmembers, nselected,
        need_bytes, nwritten, out_bytes)."""
        groups = list(groups)
        arr = (ctypes.c_int * max(len(groups), 1))(*groups)
        info = (_sz * 7)()
        if self.lib.sre_hip_lookup_lines(self.h, ptr, length, delim, arr, len(groups), keyset.h if keyset is not None else None,
                                         HIP_LINES_INVERT if invert else 0, out_ptr, out_cap, keyid_ptr, keyid_cap, index_ptr,
                                         index_cap, info, hip_stream) != 0:
            raise RuntimeError("sre_hip_lookup_lines failed")
        return LookupInfo(*info)

    def distinct_lines(self, ptr, length, out_ptr, out_cap, groups, max_keys, which=HIP_DISTINCT_FIRST, min_count=1, max_count=0,
                       delim=0x0A, invert=False, keycount_ptr=None, keycount_cap=0, keyline_ptr=None, keyline_cap=0,
                       index_ptr=None, index_cap=0, hip_stream=None):
        """sre_hip_distinct_lines: the matching lines of the device buffer (ptr, length) deduplicated by their key, the
        tuple of the texts of the capture groups `groups` of the first match.  A key qualifies when the number of lines
        that carry it, over the whole buffer, is at least min_count and (max_count != 0) at most max_count; of a
        qualifying key the call picks the first line (which=HIP_DISTINCT_FIRST), the last (HIP_DISTINCT_LAST) or every
        line (HIP_DISTINCT_EVERY), and with invert it selects the keyed lines that are not picked.  The device buffer
        (out_ptr, out_cap) receives the selected lines in line order as filter_lines writes them.  FIRST, 1, 0 is
        awk '!seen[k]++'; LAST, 1, 0 the latest record per key; FIRST, 1, 1 uniq -u; FIRST, 2, 0 uniq -d; EVERY, n, 0
        uniq -D / HAVING COUNT(*) >= n.  keycount_ptr: an optional device array of keycount_cap uint64, per line the count
        of its key or 0; keyline_ptr: an optional device array of keyline_cap int64, per line the first line of its key
        or -1; index_ptr: the filter's index rows.  The scanner's mode must be HIP_PIKE_FIRST.  Returns
        DistinctInfo(nlines, nkeyed, nkeys, nkeys_kept, nselected, need_bytes, nwritten, out_bytes).  More than max_keys
        distinct keys raise TallyOverflow, whose .info is a DistinctInfo with nlines and nkeyed and zeros elsewhere;
        nothing was written then.  Arguments the call refuses without a device raise ValueError."""
        groups = list(groups)
        if (which not in (HIP_DISTINCT_FIRST, HIP_DISTINCT_LAST, HIP_DISTINCT_EVERY) or min_count < 1
                or (max_count != 0 and max_count < min_count) or not 1 <= max_keys <= HIP_TALLY_MAX_KEYS
                or not 1 <= len(groups) <= HIP_EXTRACT_MAX_FIELDS or (keycount_cap and not keycount_ptr)
                or (keyline_cap and not keyline_ptr) or (index_cap and not index_ptr) or (out_cap and not out_ptr)):
            raise ValueError("sre_hip_distinct_lines: which, the count range, max_keys, the groups or a NULL pointer with a "
                             "capacity is out of range")
        arr = (ctypes.c_int * len(groups))(*groups)
        info = DistinctInfoStruct()
        rc = self.lib.sre_hip_distinct_lines(self.h, ptr, length, delim, arr, len(groups), which, min_count, max_count,
                                             HIP_LINES_INVERT if invert else 0, max_keys, out_ptr, out_cap, keycount_ptr,
                                             keycount_cap, keyline_ptr, keyline_cap, index_ptr, index_cap, ctypes.byref(info),
                                             hip_stream)
        res = DistinctInfo(*(getattr(info, name) for name in DistinctInfo._fields))
        if rc == HIP_TALLY_OVERFLOW:
            raise TallyOverflow(res, max_keys)
        if rc != 0:
            raise RuntimeError("sre_hip_distinct_lines failed")
        return res

    def join_lines(self, ptr, length, out_ptr, out_cap, groups, keyset, vcols, jsep=0x09, delim=0x0A, all_lines=False,
                   keyid_ptr=None, keyid_cap=0, index_ptr=None, index_cap=0, hip_stream=None):
        """sre_hip_join_lines: the lines of the device buffer (ptr, length) whose key (lookup_lines) is in the key map
        `keyset`, each followed by jsep and the value columns `vcols` of the key's dictionary row, jsep between them, and
        one delimiter, compacted in order into the device buffer (out_ptr, out_cap); with all_lines every line, the ones
        without a dictionary row with empty values.  keyid_ptr: as in lookup_lines; index_ptr: an optional device array of
        index_cap rows of 5 + 2 * len(vcols) int64: line, start, len, the row's output offset, the dictionary row (-1, -2
        as in keyid), then per column the value's output offset and length, (-1, -1) without a dictionary row.  The
        scanner's mode must be HIP_PIKE_FIRST and delim the map's.  Returns LookupInfo."""
        groups, vcols = list(groups), list(vcols)
        arr = (ctypes.c_int * max(len(groups), 1))(*groups)
        cols = (ctypes.c_int * max(len(vcols), 1))(*vcols)
        info = (_sz * 7)()
        if self.lib.sre_hip_join_lines(self.h, ptr, length, delim, arr, len(groups), keyset.h if keyset is not None else None,
                                       cols, len(vcols), jsep, HIP_LINES_ALL if all_lines else 0, out_ptr, out_cap, keyid_ptr,
                                       keyid_cap, index_ptr, index_cap, info, hip_stream) != 0:
            raise RuntimeError("sre_hip_join_lines failed")
        return LookupInfo(*info)

    def route_lines_by_key(self, ptr, length, out_ptr, out_cap, groups, keyset, delim=0x0A, all_lines=False, keyid_ptr=None,
                           keyid_cap=0, index_ptr=None, index_cap=0, buckets_ptr=None, buckets_cap=0, hip_stream=None):
        """sre_hip_route_lines_by_key: the lines of the device buffer (ptr, length) whose key (lookup_lines) is in the KeySet
        `keyset`, grouped by the key's dictionary row: the device buffer (out_ptr, out_cap) receives the lines of the lowest
        row first, in line order, then the next row's, .., each followed by one delimiter.  With all_lines every line: the
        keyed lines whose key the set does not hold (id -1) follow the last row's, the lines without a key (id -2) come
        last.  keyid_ptr: as in lookup_lines; index_ptr: an optional device array of index_cap rows [line no, offset in the
        buffer, length, offset in the output, id] in output order; buckets_ptr: an optional device array of buckets_cap
        rows [id, rank of the first line, lines, offset in the full output, bytes], one per non-empty bucket in output
        order, complete whatever out_cap is.  The scanner's mode must be HIP_PIKE_FIRST.  Returns RouteKeyInfo(nlines,
        nkeyed, nmembers, nselected, nbuckets, need_bytes, nwritten, out_bytes)."""
        groups = list(groups)
        arr = (ctypes.c_int * max(len(groups), 1))(*groups)
        info = (_sz * 8)()
        if self.lib.sre_hip_route_lines_by_key(self.h, ptr, length, delim, arr, len(groups), keyset.h if keyset is not None else None,
                                               HIP_LINES_ALL if all_lines else 0, out_ptr, out_cap, keyid_ptr, keyid_cap, index_ptr,
                                               index_cap, buckets_ptr, buckets_cap, info, hip_stream) != 0:
            raise RuntimeError("sre_hip_route_lines_by_key failed")
        return RouteKeyInfo(*info)

    def sort_lines(self, ptr, length, out_ptr, out_cap, group, delim=0x0A, descending=False, all_lines=False, limit=0,
                   index_ptr=None, index_cap=0, hip_stream=None):
        """sre_hip_sort_lines: the lines of the device buffer (ptr, length) whose capture group `group` of the first match is
        a number (tally_number's rule), ordered by that number, ascending or (descending) largest first; equal values stay
        in line order either way.  The device buffer (out_ptr, out_cap) receives them, each followed by one delimiter.
        With all_lines every line: the lines that are not numbered follow all numbered ones in line order.  limit != 0
        keeps the first `limit` rows of that order.  index_ptr: an optional device array of index_cap rows [line no, offset
        in the buffer, length, offset in the output, value, class (1 numbered, -1 keyed but no number, -2 no match)] in
        output order.  The sort is stable, so sorting the output again by another group orders by (second, first, line).
        The scanner's mode must be HIP_PIKE_FIRST.  Returns SortInfo(nlines, nkeyed, nnumbered, nselected, need_bytes,
        nwritten, out_bytes, passes, vmin, vmax)."""
        info = SortInfoStruct()
        flags = (HIP_LINES_ALL if all_lines else 0) | (HIP_SORT_DESC if descending else 0)
        if self.lib.sre_hip_sort_lines(self.h, ptr, length, delim, group, flags, limit, out_ptr, out_cap, index_ptr, index_cap,
                                       ctypes.byref(info), hip_stream) != 0:
            raise RuntimeError("sre_hip_sort_lines failed")
        return SortInfo(*(getattr(info, name) for name in SortInfo._fields))

    def sort_lines_text(self, ptr, length, out_ptr, out_cap, group, delim=0x0A, max_bytes=0, descending=False, all_lines=False,
                        limit=0, index_ptr=None, index_cap=0, hip_stream=None):
        """sre_hip_sort_lines_text: the lines of the device buffer (ptr, length) that have a match, ordered by the bytes of
        capture group `group` of the first match (memcmp order, a proper prefix first; an unset group is the empty text),
        ascending or descending; equal texts stay in line order either way.  max_bytes != 0 compares only the first
        max_bytes bytes.  The device buffer (out_ptr, out_cap) receives the lines, each followed by one delimiter.  With
        all_lines every line: the lines without a match follow all others in line order.  limit != 0 keeps the first
        `limit` rows of that order.  index_ptr: an optional device array of index_cap rows [line no, offset in the buffer,
        length, offset in the output, offset of the field in the buffer, its full length], the last two -1, -1 for an
        unset group or a line without a match.  The sort is stable, so sorting the output again by another group, by text
        or with sort_lines, orders by (second, first, line).  The cost is linear in the longest compared text
        (sort_text_plan lists the passes).  The scanner's mode must be HIP_PIKE_FIRST.  Returns SortTextInfo(nlines,
        nkeyed, nselected, need_bytes, nwritten, out_bytes, passes, minlen, maxlen)."""
        info = SortTextInfoStruct()
        flags = (HIP_LINES_ALL if all_lines else 0) | (HIP_SORT_DESC if descending else 0)
        if self.lib.sre_hip_sort_lines_text(self.h, ptr, length, delim, group, max_bytes, flags, limit, out_ptr, out_cap, index_ptr,
                                            index_cap, ctypes.byref(info), hip_stream) != 0:
            raise RuntimeError("sre_hip_sort_lines_text failed")
        return SortTextInfo(*(getattr(info, name) for name in SortTextInfo._fields))

    def tally_top_lines(self, ptr, length, out_ptr, out_cap, groups, vgroups, max_keys, by=HIP_TOP_COUNT, by_col=0,
                        descending=True, limit=0, delim=0x0A, fsep=0x09, all_lines=False, counts_ptr=None, counts_cap=0,
                        sums_ptr=None, sums_cap=0, rank_ptr=None, rank_cap=0, index_ptr=None, index_cap=0, hip_stream=None):
        """sre_hip_tally_top_lines: tally_sums_lines whose rows, counts, aggregates and index rows come out ordered by the
        keys' order value: the count (by=HIP_TOP_COUNT), or the n / sum / min / max of value column by_col (HIP_TOP_N,
        _SUM, _MIN, _MAX), descending or ascending; keys of equal value stay in first-appearance order either way, and
        the keys whose column holds no number (SUM, MIN, MAX only) follow all others.  limit != 0 keeps the first
        `limit` rows of that order.  vgroups may be empty with by=HIP_TOP_COUNT and no sums.  counts_ptr / sums_ptr: as
        in tally_sums_lines, row r the key at rank r; index_ptr: an optional device array of index_cap rows of 6 + 2 *
        len(groups) int64, the extract's index row of the key's first line with [3] the row's offset in this output, then
        the key's number in first-appearance order and its order value; rank_ptr: an optional device array of rank_cap
        int64, the rank of line i's key in the full order or -1.  Returns TallyTopInfo(nlines, nselected, nkeys,
        nordered, nrows, need_bytes, nwritten, out_bytes, passes, vmin, vmax); raises TallyOverflow as tally_lines does,
        with nothing written."""
        groups, vgroups = list(groups), list(vgroups or ())
        arr = (ctypes.c_int * max(len(groups), 1))(*groups)
        varr = (ctypes.c_int * len(vgroups))(*vgroups) if vgroups else None
        info = TallyTopInfoStruct()
        flags = (HIP_LINES_ALL if all_lines else 0) | (HIP_SORT_DESC if descending else 0)
        rc = self.lib.sre_hip_tally_top_lines(self.h, ptr, length, delim, arr, len(groups), varr, len(vgroups), fsep, flags,
                                              max_keys, by, by_col, limit, out_ptr, out_cap, counts_ptr, counts_cap, sums_ptr,
                                              sums_cap, rank_ptr, rank_cap, index_ptr, index_cap, ctypes.byref(info), hip_stream)
        res = TallyTopInfo(*(getattr(info, name) for name in TallyTopInfo._fields))
        if rc == HIP_TALLY_OVERFLOW:
            raise TallyOverflow(TallyInfo(res.nlines, res.nselected, 0, 0, 0, 0), max_keys)
        if rc != 0:
            raise RuntimeError("sre_hip_tally_top_lines failed")
        return res

    @property
    def last_line_batches(self):
        return self.lib.sre_hip_scanner_last_line_batches(self.h)

    @property
    def last_lines_device(self):
        """1 when every batch of the last scan_lines call ran on the device with no per-line host work"""
        return self.lib.sre_hip_scanner_last_lines_device(self.h)

    @property
    def last_short_lines(self):
        """lines of the last scan_lines call that the NFA tier's short-line kernel took"""
        return self.lib.sre_hip_scanner_last_short_lines(self.h)


FilterInfo = collections.namedtuple("FilterInfo", "nlines nselected need_bytes nwritten out_bytes")
RouteBucket = collections.namedtuple("RouteBucket", "nlines offset bytes")
ContextInfo = collections.namedtuple("ContextInfo", "nlines nmatched nselected ngroups need_bytes nwritten out_bytes")
TallyInfo = collections.namedtuple("TallyInfo", "nlines nselected nkeys need_bytes nwritten out_bytes")
LookupInfo = collections.namedtuple("LookupInfo", "nlines nkeyed nmembers nselected need_bytes nwritten out_bytes")
RouteKeyInfo = collections.namedtuple("RouteKeyInfo", "nlines nkeyed nmembers nselected nbuckets need_bytes nwritten out_bytes")
SortInfo = collections.namedtuple("SortInfo", "nlines nkeyed nnumbered nselected need_bytes nwritten out_bytes passes vmin vmax")


TallyTopInfo = collections.namedtuple("TallyTopInfo", "nlines nselected nkeys nordered nrows need_bytes nwritten out_bytes passes vmin vmax")


class TallyTopInfoStruct(ctypes.Structure):
    """sre_hip_tally_top_info_t"""
    _fields_ = [(name, ctypes.c_int64 if name in ("vmin", "vmax") else ctypes.c_size_t) for name in TallyTopInfo._fields]


SortTextInfo = collections.namedtuple("SortTextInfo", "nlines nkeyed nselected need_bytes nwritten out_bytes passes minlen maxlen")


class SortTextInfoStruct(ctypes.Structure):
    """sre_hip_sort_text_info_t"""
    _fields_ = [(name, ctypes.c_size_t) for name in SortTextInfo._fields]


class SortInfoStruct(ctypes.Structure):
    """sre_hip_sort_info_t"""
    _fields_ = [(name, ctypes.c_int64 if name in ("vmin", "vmax") else ctypes.c_size_t) for name in SortInfo._fields]


DistinctInfo = collections.namedtuple("DistinctInfo", "nlines nkeyed nkeys nkeys_kept nselected need_bytes nwritten out_bytes")


class DistinctInfoStruct(ctypes.Structure):
    """sre_hip_distinct_info_t"""
    _fields_ = [(name, ctypes.c_size_t) for name in DistinctInfo._fields]


FoldInfo = collections.namedtuple("FoldInfo", "nlines nmarked nrecords longest need_bytes nwritten out_bytes")


class FoldInfoStruct(ctypes.Structure):
    """sre_hip_fold_info_t"""
    _fields_ = [(name, ctypes.c_size_t) for name in FoldInfo._fields]


class TallyInfoStruct(ctypes.Structure):
    """sre_hip_tally_info_t"""
    _fields_ = [(name, ctypes.c_size_t) for name in TallyInfo._fields]


class TallySumStruct(ctypes.Structure):
    """sre_hip_tally_sum_t"""
    _fields_ = [("sum", ctypes.c_int64), ("min", ctypes.c_int64), ("max", ctypes.c_int64), ("n", ctypes.c_uint64)]


class TallyOverflow(RuntimeError):
    """sre_hip_tally_lines returned SRE_HIP_TALLY_OVERFLOW: the buffer holds more than max_keys distinct keys.  .info is
    the call's TallyInfo (nlines and nselected, zeros elsewhere)."""

    def __init__(self, info, max_keys):
        RuntimeError.__init__(self, "sre_hip_tally_lines: more than max_keys = %d distinct keys" % max_keys)
        self.info = info
        self.max_keys = max_keys


class StreamSet:
    """sre_hip_streams_* (include/sregex_hip.h): n streams of one program whose contexts live on
    the device and are fed chunk by chunk, all together in one call."""

    OPEN, CLOSED, WAS_CLOSED, NOT_FED = 0, 1, 2, 3

    def __init__(self, pool, prog, mode, nstreams, engine=None):
        """engine: None = sre_hip_streams_create (the table-driven scanner); ENGINE_AUTO / ENGINE_SCAN /
        ENGINE_NFA = sre_hip_streams_create_engine (the NFA tier: HIP_THOMPSON, no look-ahead assertions)"""
        self.lib = pool.lib
        if engine is None:
            self.h = self.lib.sre_hip_streams_create(pool.p, prog.h, mode, nstreams)
        else:
            self.h = self.lib.sre_hip_streams_create_engine(pool.p, prog.h, mode, engine, nstreams)
        if not self.h:
            raise RuntimeError("sre_hip_streams_create%s failed (no HIP device, or the program's chunks "
                               "do not run on the engine asked for)" % ("" if engine is None else "_engine"))
        self.n = self.lib.sre_hip_streams_count(self.h)
        self.slots = self.lib.sre_hip_streams_result_slots(self.h)
        self._out = (ctypes.c_ssize_t * (self.n * self.slots))()

    def feed_raw(self, ptrs, lens, eof, hip_stream=None):
        """one call with ctypes arrays of n entries; returns the flat ctypes array of records"""
        if self.lib.sre_hip_streams_feed(self.h, ptrs, lens, eof, self._out, hip_stream) != 0:
            raise RuntimeError("sre_hip_streams_feed failed")
        return self._out

    def feed(self, ptrs, lens, eof, hip_stream=None):
        """ptrs[i]: device pointer of stream i's chunk, or None (not fed in this call); returns one
        record [rc, state, has_pending, pending0, pending1, ovector...] per stream"""
        n = self.n
        if not (len(ptrs) == len(lens) == len(eof) == n):
            raise ValueError("a stream set of %d streams takes %d pointers, lengths and eof flags" % (n, n))
        out = self.feed_raw((_vp * n)(*ptrs), (_sz * n)(*lens), (ctypes.c_ubyte * n)(*[1 if e else 0 for e in eof]),
                            hip_stream)
        s = self.slots
        return [list(out[i * s:(i + 1) * s]) for i in range(n)]

    def reset(self, idx):
        idx = list(idx)
        if self.lib.sre_hip_streams_reset(self.h, (_sz * max(len(idx), 1))(*idx), len(idx)) != 0:
            raise RuntimeError("sre_hip_streams_reset failed")

    @property
    def device_bytes(self):
        return self.lib.sre_hip_streams_device_bytes(self.h)

    @property
    def last_fixups(self):
        return self.lib.sre_hip_streams_last_fixups(self.h)

    @property
    def last_launches(self):
        return self.lib.sre_hip_streams_last_launches(self.h)

    @property
    def engine(self):
        return self.lib.sre_hip_streams_engine(self.h)

    @property
    def nfa_bits(self):
        return self.lib.sre_hip_streams_nfa_bits(self.h)

    @property
    def last_exact_passes(self):
        return self.lib.sre_hip_streams_last_exact_passes(self.h)


class DeviceBuffer:
    """A device allocation made through the library (no torch needed)."""

    def __init__(self, nbytes, lib=None):
        self.lib = lib or load_library()
        self.nbytes = nbytes
        self.ptr = self.lib.sre_hip_alloc(nbytes)
        if not self.ptr:
            raise RuntimeError("sre_hip_alloc(%d) failed" % nbytes)

    @classmethod
    def from_bytes(cls, data, lib=None):
        b = cls(max(len(data), 1), lib)
        if len(data) and b.lib.sre_hip_upload(b.ptr, bytes(data), len(data)) != 0:
            raise RuntimeError("sre_hip_upload failed")
        b.nbytes = len(data)
        return b

    def to_bytes(self, n=None):
        n = self.nbytes if n is None else n
        out = ctypes.create_string_buffer(n)
        if n and self.lib.sre_hip_download(out, self.ptr, n) != 0:
            raise RuntimeError("sre_hip_download failed")
        return out.raw

    def free(self):
        if self.ptr:
            self.lib.sre_hip_free(self.ptr)
            self.ptr = None


def compat_route_counts():
    """(whole buffer on a scanner, chunk on the table-driven scanner, exact VM) exec calls so far"""
    out = (ctypes.c_ulonglong * 3)()
    load_library().sre_hip_compat_route_counts(out)
    return tuple(out)


def gen_data_length(n, tail_len):
    """Length of stream(n, tail) = "abccc" x floor((n - tail_len) / 5) + tail
    (reference bench/gen-data.pl:9)."""
    return ((n - tail_len) // 5) * 5 + tail_len


def gen_data_host(n, tail):
    """The same stream on the host (tests, CPU baseline)."""
    return b"abccc" * ((n - len(tail)) // 5) + bytes(tail)
