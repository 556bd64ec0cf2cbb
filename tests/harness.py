"""Shared test plumbing: golden loaders, the oracle binding, and a driver that
replays the reference CLI's per-subject call sequence (reference
src/sre_cli.c:298-660 `process_string`) against any engine.

`oracle/` is test infrastructure; this module (under tests/) is one of the few
places allowed to load it.
"""
import ctypes
import gzip
import json
import os
import subprocess

import sregex_amd as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
ORACLE_DIR = os.path.join(ROOT, "oracle")
FORCE_RE = "^章亦春$".encode("utf-8")

_vp, _sz, _ssz = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_ssize_t
_pssz = ctypes.POINTER(ctypes.c_ssize_t)


# ------------------------------------------------------------------ goldens

def load_blocks():
    with gzip.open(os.path.join(GOLDEN, "t_blocks.jsonl.gz"), "rt") as f:
        return [json.loads(l) for l in f]


def load_jsonl(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return [json.loads(l) for l in f]


def parse_flags(s, n):
    """reference src/sre_cli.c:680-711: space advances to the next regex, 'i' = caseless"""
    fl = [0] * n
    i = 0
    for ch in s or "":
        if ch == " ":
            i += 1
        elif ch == "i":
            fl[i] |= S.SRE_REGEX_CASELESS
    return fl


def block_variants(blk):
    """(variant name, regex list, flags list, multi?, reference record)"""
    res = [bytes.fromhex(h) for h in blk["re"]]
    flags = blk.get("flags", "")
    out = [("ref", res, parse_flags(flags, len(res)), bool(blk["multi"]), blk["ref"])]
    if "ref_multi" in blk:
        mres = [FORCE_RE] + res
        out.append(("ref_multi", mres, parse_flags((" " + flags) if flags else "", len(mres)),
                    True, blk["ref_multi"]))
    return out


# ------------------------------------------------------------------ oracle

_oracle = None


def oracle_lib():
    """liboracle.so = CPU restatement of the reference VMs (oracle/*.c)."""
    global _oracle
    if _oracle is None:
        so = os.path.join(ORACLE_DIR, "liboracle.so")
        if not os.path.exists(so):
            subprocess.check_call(["make", "-C", ORACLE_DIR, "port"], stdout=subprocess.DEVNULL)
        L = ctypes.CDLL(so)
        L.sre_oracle_pike_create_ctx.restype = _vp
        L.sre_oracle_pike_create_ctx.argtypes = [_vp, _pssz, _sz]
        L.sre_oracle_pike_exec.restype = _ssz
        L.sre_oracle_pike_exec.argtypes = [_vp, _vp, _sz, ctypes.c_uint, ctypes.POINTER(_pssz)]
        L.sre_oracle_pike_free.argtypes = [_vp]
        L.sre_oracle_thompson_create_ctx.restype = _vp
        L.sre_oracle_thompson_create_ctx.argtypes = [_vp]
        L.sre_oracle_thompson_exec.restype = _ssz
        L.sre_oracle_thompson_exec.argtypes = [_vp, _vp, _sz, ctypes.c_uint]
        L.sre_oracle_thompson_free.argtypes = [_vp]
        L.sre_oracle_pike_count.restype = _ssz
        L.sre_oracle_pike_count.argtypes = [_vp, _vp, _sz, _pssz, _sz, _sz, _pssz]
        _oracle = L
    return _oracle


class _OraclePike:
    def __init__(self, prog, ncaps):
        self.L = oracle_lib()
        n = 2 * (ncaps + 1)
        self.ovector = (ctypes.c_ssize_t * n)(*([0] * n))
        self.h = self.L.sre_oracle_pike_create_ctx(prog.h, self.ovector, n * 8)
        self.pending = None

    def exec(self, data, eof, want_pending=True, base=None, offset=0, length=None):
        if base is not None:
            ptr, n, keep = ctypes.cast(ctypes.addressof(base) + offset, _vp), length, base
        else:
            ptr, n, keep = S._as_buffer(data)
        pend = _pssz()
        rc = self.L.sre_oracle_pike_exec(self.h, ptr, n, 1 if eof else 0,
                                         ctypes.byref(pend) if want_pending else None)
        self.pending = (pend[0], pend[1]) if (want_pending and rc == S.SRE_AGAIN and pend) else None
        del keep
        return rc

    def close(self):
        self.L.sre_oracle_pike_free(self.h)
        self.h = None


class _OracleThompson:
    def __init__(self, prog):
        self.L = oracle_lib()
        self.h = self.L.sre_oracle_thompson_create_ctx(prog.h)

    def exec(self, data, eof):
        ptr, n, keep = S._as_buffer(data)
        rc = self.L.sre_oracle_thompson_exec(self.h, ptr, n, 1 if eof else 0)
        del keep
        return rc

    def close(self):
        self.L.sre_oracle_thompson_free(self.h)
        self.h = None


class OracleEngine:
    name = "oracle"

    def pike(self, prog, ncaps):
        return _OraclePike(prog, ncaps)

    def thompson(self, prog):
        return _OracleThompson(prog)

    def count(self, prog, data, nov, max_spans=0):
        L = oracle_lib()
        spans = (ctypes.c_ssize_t * (max(max_spans, 1) * (nov + 1)))()
        buf = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
        final = ctypes.c_ssize_t(0)
        n = L.sre_oracle_pike_count(prog.h, ctypes.cast(buf, _vp), len(data), spans, nov, max_spans,
                                    ctypes.byref(final))
        got = [list(spans[i * (nov + 1):(i + 1) * (nov + 1)]) for i in range(min(n, max_spans))]
        self.final_rc = final.value
        return n, got


class ProductEngine:
    """The product through its C ABI (HIP kernels behind sre_vm_*_exec)."""
    name = "product"

    def __init__(self):
        self.pool = S.Pool()

    def pike(self, prog, ncaps):
        c = S.PikeCtx(self.pool, prog, ncaps)
        c.close = lambda: None
        return c

    def thompson(self, prog):
        c = S.ThompsonCtx(self.pool, prog)
        c.close = lambda: None
        return c

    def recycle(self):
        """Free per-context device state between subjects (the CLI destroys its
        exec pool per subject, src/sre_cli.c:657)."""
        self.pool.destroy()
        self.pool = S.Pool()


# ------------------------------------------------------------------ CLI replay

_RC_WORD = {S.SRE_AGAIN: "again", S.SRE_DECLINED: "no match", S.SRE_ERROR: "error"}


def _fmt_caps(ov, n):
    return "".join(" (%d, %d)" % (ov[i], ov[i + 1]) for i in range(0, n, 2))


def cli_lines(engine, prog, subject, ncaps):
    """The four engine lines the reference CLI prints for one subject that do
    not involve the (dropped) JIT: thompson, splitted thompson, pike, splitted
    pike — same call sequence and formatting as src/sre_cli.c:313-656."""
    out = []
    nov = 2 * (ncaps + 1)

    # thompson, whole buffer (:327-355)
    t = engine.thompson(prog)
    rc = t.exec(subject, True)
    out.append("thompson " + ("match" if rc == S.SRE_OK else _RC_WORD.get(rc, "rc=%d" % rc)))
    t.close()

    # splitted thompson: alternate an empty chunk and a 1-byte chunk (:361-411)
    t = engine.thompson(prog)
    line = None
    for i in range(len(subject)):
        for chunk in (b"", subject[i:i + 1]):
            rc = t.exec(chunk, False)
            if rc != S.SRE_AGAIN:
                break
        if rc != S.SRE_AGAIN:
            break
    else:
        rc = t.exec(b"", True)
    line = "match" if rc == S.SRE_OK else _RC_WORD.get(rc, "rc=%d" % rc)
    out.append("splitted thompson " + line)
    t.close()

    # pike, whole buffer (:537-566)
    p = engine.pike(prog, ncaps)
    rc = p.exec(subject, True, want_pending=False)
    if rc >= 0:
        out.append("pike match %d%s" % (rc, _fmt_caps(p.ovector, nov)))
    else:
        out.append("pike " + _RC_WORD.get(rc, "unknown (%d)" % rc))
    p.close()

    # splitted pike (:570-656): temp captures "[(a, b)]" and pending "(a, b) "
    # are printed for every 1-byte chunk that answers AGAIN
    p = engine.pike(prog, ncaps)
    s = ""
    done = False
    for i in range(len(subject)):
        rc = p.exec(b"", False, want_pending=False)
        if rc == S.SRE_AGAIN:
            rc = p.exec(subject[i:i + 1], False, want_pending=True)
            if rc == S.SRE_AGAIN:
                s += "[(%d, %d)]" % (p.ovector[0], p.ovector[1])
                s += ("(%d, %d) " % p.pending) if p.pending else " "
                continue
        done = True
        break
    if not done:
        rc = p.exec(b"", True, want_pending=True)
    if rc >= 0:
        s += "match %d%s" % (rc, _fmt_caps(p.ovector, nov))
    else:
        s += _RC_WORD.get(rc, "unknown (%d)" % rc)
    out.append("splitted pike " + s)
    p.close()
    return out


def ref_lines(ref):
    """The same four lines out of a golden record (res[] = the CLI's six lines)."""
    r = ref["res"]
    return [r[0], r[1], r[4], r[5]]


def findall(engine, prog, ncaps, data, limit=1 << 30):
    """Iterate exec on ONE context, re-feeding from each match end."""
    p = engine.pike(prog, ncaps)
    nov = 2 * (ncaps + 1)
    base = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    off, out = 0, []
    while len(out) < limit:
        rc = p.exec(None, True, want_pending=False, base=base, offset=off, length=len(data) - off)
        if rc < 0:
            out.append([rc])
            break
        out.append([rc] + list(p.ovector[:nov]))
        off = p.ovector[1]
    p.close()
    return out


# ------------------------------------------------------------------ random patterns

def random_regex(rng, depth=0, wide=None):
    """A random pattern over a small alphabet, from the constructs the reference
    parser accepts: literals, classes, '.', groups, alternation, greedy and lazy
    quantifiers, counted repeats, and every assertion."""
    atoms = [b"a", b"b", b"c", b"x", b".", b"[ab]", b"[^a]", b"\\w", b"\\s", b"\\n", b"[a-c]"]
    if wide is None:
        wide = bool(os.environ.get("SRE_FUZZ_WIDE"))
    if wide:
        # more of the lexer: escapes, negated shorthands, upper case (for caseless flags), high bytes
        atoms += [b"A", b"X", b"\\.", b"\\W", b"\\S", b"\\d", b"\\D", b"[^\\s]", b"[\\w.]", b"\\x41",
                  b"\\xff", b"[\\x80-\\xff]", b"_", b"[A-C]"]
    asserts = [b"^", b"$", b"\\b", b"\\B", b"\\A", b"\\z"]
    n = rng.randrange(1, 5 if depth == 0 else 4)
    seq = []
    for _ in range(n):
        r = rng.random()
        if r < 0.12:
            piece = rng.choice(asserts)
        elif r < 0.30 and depth < 2:
            inner = random_regex(rng, depth + 1, wide)
            if rng.random() < 0.5:
                inner += b"|" + random_regex(rng, depth + 1, wide)
            piece = (b"(" if rng.random() < 0.7 else b"(?:") + inner + b")"
        else:
            piece = rng.choice(atoms)
        if piece not in asserts and rng.random() < 0.45:
            piece += rng.choice([b"*", b"+", b"?", b"*?", b"+?", b"??", b"{2}", b"{1,3}", b"{0,2}?"])
        seq.append(piece)
    return b"".join(seq)


# ------------------------------------------------------------------ the scanner's 8-bit index form

# The scan kernel indexes its fast table with packed byte classes (1, 2 or 4 bits each) up to 16 classes and
# with the input byte itself above that.  This alternative adds 17 byte classes to any program and leaves the
# rest of it alone, so a padded program has more than 16 (tests/test_gpu_scan_forms.py, tests/test_scan_model.py).
SCAN_PAD = b"|0123456789ABCDEFG"


def pad_into_8bit_form(pats):
    """the same regexes, the first one with the SCAN_PAD alternative"""
    return [pats[0] + SCAN_PAD] + list(pats[1:])


def padded_subject(rng, size, alphabet=b"abcx \n_."):
    """`size` random bytes over the alphabet and, with probability 1/2, one insertion at a random position: the
    pad's literal, a prefix of it, or one of the bytes 0x00 0x80 0xff"""
    d = bytearray(rng.choice(alphabet) for _ in range(size))
    if rng.random() < 0.5:
        lit = SCAN_PAD[1:]
        ins = rng.choice([lit, lit[:rng.randrange(1, len(lit))], bytes([rng.choice(b"\x00\x80\xff")])])
        at = rng.randrange(0, len(d) + 1)
        d[at:at] = ins
    return bytes(d)


# ------------------------------------------------------------------ recorded replies of the reference

# The randomised differential tests (test_frontend_fuzz.py, test_oracle.py's live differential) put
# their inputs to the real reference.  Its replies to the inputs of the fixed seeds are recorded in
# tests/golden/reference_fuzz.jsonl.gz (tests/golden/make_goldens.py --fuzz-only, from oracle/_ref),
# so that these tests run without the reference; an input without a recorded reply (another
# SRE_FUZZ_SEED) is put to the live reference in oracle/_ref, when that is built.
REF_DIR = os.path.join(ORACLE_DIR, "_ref")
REF_CLI = os.path.join(REF_DIR, "sregex-cli")
REF_SO = os.path.join(REF_DIR, "libsregex_ref.so")
REPLIES = "reference_fuzz.jsonl.gz"
FUZZ_SEED = 99                  # test_frontend_fuzz.py's sequence unless SRE_FUZZ_SEED says otherwise
LIVE_DIFF_SEED = 20261004       # test_oracle.py's live differential


def reply_key(kind, pats, *rest):
    return json.dumps([kind, [p.hex() for p in pats]] + [r.hex() if isinstance(r, bytes) else r for r in rest])


_replies = None


def recorded_replies():
    global _replies
    if _replies is None:
        with gzip.open(os.path.join(GOLDEN, REPLIES), "rt") as f:
            _replies = {r["k"]: r["v"] for r in map(json.loads, f)}
    return _replies


def reference_reply(key, live, needs):
    """the recorded reply to `key`, else live() when the reference binary `needs` is built"""
    rec = recorded_replies()
    if key in rec:
        return rec[key]
    if not os.path.exists(needs):
        import pytest
        pytest.skip("no recorded reply of the reference to this input (another SRE_FUZZ_SEED?) "
                    "and %s is not built" % os.path.relpath(needs, ROOT))
    return live()


def cli_parse_reply(pat, caseless=False):
    """AST dump / capture count / program dump of one pattern, or its syntax error, as the reference
    CLI prints them; None where the reference crashed or the argument is not taken as a pattern"""
    try:
        p = subprocess.run([REF_CLI] + (["--flags", "i"] if caseless else []) + [pat, b""], capture_output=True,
                           timeout=20)
    except subprocess.TimeoutExpired:
        return None
    if p.returncode < 0:
        return None                      # the reference crashed on this one
    err = p.stderr.decode("latin-1").strip()
    if "[error]" in err:
        return {"err": err.splitlines()[0]}
    if p.returncode != 0 and not p.stdout:
        return None                      # an option-like argument, not a pattern
    out = p.stdout.decode("latin-1").split("\n## ")[0].split("\n")
    return {"ast": out[0], "ncaps": int(out[1].split(":")[1]), "prog": "\n".join(out[2:]).rstrip("\n")}


def cli_exec_reply(pats, subject):
    """the reference CLI's thompson / splitted thompson / pike / splitted pike lines for the subject
    (its JIT lines left out); None where the reference crashed or timed out"""
    argv = [REF_CLI] + (["-n", str(len(pats))] if len(pats) > 1 else []) + pats + [subject]
    try:
        p = subprocess.run(argv, capture_output=True, timeout=20)
    except subprocess.TimeoutExpired:
        return None
    if p.returncode != 0:
        return None                      # the reference crashes on some programs
    # the six engine lines close the output (the subject itself may hold newlines)
    lines = [l for l in p.stdout.decode("latin-1").split("\n") if l][-6:]
    return [l for l in lines if "jitted" not in l]


def frontend_fuzz_cases(seed):
    """test_frontend_fuzz.py: random and randomly damaged patterns (SRE_FUZZ_WIDE atoms), and
    whether the caseless flag is given"""
    import random
    rng = random.Random(seed)
    junk = b"()[]{}*+?|\\^$.,-0123456789abx:=!<>"
    for _ in range(1200):
        pat = random_regex(rng, wide=True)
        if rng.random() < 0.4:           # damage it: insert / delete / replace a byte
            b = bytearray(pat)
            for _ in range(rng.randrange(1, 3)):
                k = rng.randrange(0, len(b) + 1)
                op = rng.randrange(3)
                if op == 0 or not b:
                    b.insert(k, rng.choice(junk))
                elif op == 1:
                    del b[min(k, len(b) - 1)]
                else:
                    b[min(k, len(b) - 1)] = rng.choice(junk)
            pat = bytes(b)
        if not pat or b"\0" in pat or pat.startswith(b"-"):
            continue
        caseless = rng.random() < 0.3       # applied at parse time (sre_yyparser.y:244-279, sre_regex.c:170-214)
        yield pat, caseless


def oracle_fuzz_cases(seed):
    """test_frontend_fuzz.py: random patterns (one, or two or three of them) and subjects"""
    import random
    rng = random.Random(seed + 1000)
    alphabet = b"abcx \n_."
    for _ in range(500):
        pats = [random_regex(rng) for _ in range(1 if rng.random() < 0.75 else rng.randrange(2, 4))]
        if any(p.startswith(b"-") for p in pats):
            continue
        subject = bytes(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 3, 9, 20, 33])))
        if subject.startswith(b"-"):
            continue
        yield pats, subject


LIVE_DIFF_ZOO = [
    [rb"(a*)*b"], [rb"(a*)+"], [rb"(a|b)*?c"], [rb"\bfoo\b"], [rb"^a|b$"], [rb"a$|ab"],
    [rb"(?:a$|a)b?"], [rb"\Ba\B|c\b"], [rb"(a+)(b+)?"], [rb"x*"], [rb"(|a)+"], [rb"a{2,3}b{0,2}"],
    [rb"\Aab|\n^b"], [rb"[^a]\z|a"], [rb"a", rb"ab", rb"\s+", rb"b$"], [rb"(a)|b", rb"(b)(c)?"],
    [rb"$"], [rb"^"], [rb"\b"], [rb"(a?)*?b"], [rb"((a)|b)+"], [rb"a.c"], [rb"[a-c]+\.[^b]"],
]


def live_differential_cases():
    """test_oracle.py: a pattern zoo that leans on assertions, empty matches, nested stars and
    multi-regex, each with 60 random subjects over a small alphabet"""
    import random
    rng = random.Random(LIVE_DIFF_SEED)
    alphabet = b"ab c\n.x"
    for pats in LIVE_DIFF_ZOO:
        yield pats, [bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 24))) for _ in range(60)]
