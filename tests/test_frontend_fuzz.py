"""Front end (parser + compiler) against the reference CLI on random and
randomly damaged patterns: its replies to the fixed seed's inputs are recorded
in tests/golden/reference_fuzz.jsonl.gz (tests/golden/make_goldens.py
--fuzz-only), another SRE_FUZZ_SEED asks the live CLI (oracle/_ref/sregex-cli,
the real reference compiled by oracle/Makefile).  Compared: AST dump, capture
count, program dump — or the syntax-error offset."""
import os

import sregex_amd as S
import harness


def _ours(pat, caseless=False):
    with S.Pool() as pool:
        try:
            re = S.parse(pool, [pat], [S.SRE_REGEX_CASELESS] if caseless else None)
        except S.SyntaxError_ as e:
            return {"err": str(e)}
        prog = S.compile(pool, re)
        return {"ast": re.dump().rstrip("\n"), "ncaps": re.ncaps, "prog": prog.dump().rstrip("\n")}


def _theirs(pat, caseless=False):
    return harness.reference_reply(harness.reply_key("parse", [pat], caseless),
                                   lambda: harness.cli_parse_reply(pat, caseless), harness.REF_CLI)


def test_random_and_damaged_patterns_parse_like_the_reference():
    bad = []
    n = crashed = rejected = 0
    for pat, caseless in harness.frontend_fuzz_cases(int(os.environ.get("SRE_FUZZ_SEED", harness.FUZZ_SEED))):
        want = _theirs(pat, caseless)
        if want is None:
            crashed += 1
            continue
        got = _ours(pat, caseless)
        n += 1
        rejected += "err" in want
        if got != want:
            bad.append((pat, got.get("err") or got.get("ast"), want.get("err") or want.get("ast")))
    assert n > 1000 and rejected > 50, (n, rejected, crashed)
    assert not bad, (len(bad), bad[:5])


def test_oracle_matches_the_live_reference_on_random_patterns():
    """The oracle (oracle/*.c) against the real reference executors (their recorded
    replies), through the reference CLI's own call sequence: thompson / splitted thompson / pike /
    splitted pike lines (captures, temp captures, pending matches) on random
    patterns — assertions, lazy quantifiers, counted repeats — and subjects."""
    ora = harness.OracleEngine()
    bad = []
    n = crashed = 0
    for pats, subject in harness.oracle_fuzz_cases(int(os.environ.get("SRE_FUZZ_SEED", harness.FUZZ_SEED))):
        pat = pats
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            want = harness.reference_reply(harness.reply_key("exec", pats, subject),
                                           lambda: harness.cli_exec_reply(pats, subject), harness.REF_CLI)
            if want is None:
                crashed += 1                # the reference crashes on some programs
                continue
            got = harness.cli_lines(ora, prog, subject, re.ncaps)
            n += 1
            if got != want:
                bad.append((pat, subject, got, want))
    assert n > 400, (n, crashed)
    assert not bad, (len(bad), bad[:3])
