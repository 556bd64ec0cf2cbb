"""Pin the CPU restatement (oracle/) against the reference before anything
trusts it:

  (a) every block of the reference's t/ suite, single and forced-multi form,
      whole-buffer and byte-at-a-time ("splitted") modes, Thompson and Pike —
      compared with the lines the reference's own CLI printed
      (tests/golden/t_blocks.jsonl.gz, made by tests/golden/make_goldens.py);
  (b) the explicit expectations stored in the .t files themselves
      (`--- cap`, `--- match_id`, `--- temp_cap`, `--- no_match`);
  (c) reference runs over gen-data streams and find-all iteration traces;
  (d) differential runs against the real reference library on random subjects
      (its replies recorded in tests/golden/reference_fuzz.jsonl.gz).
"""
import os

import sregex_amd as S
import harness

ENG = harness.OracleEngine()


def test_all_reference_blocks_whole_and_splitted(lib, blocks):
    bad, n = [], 0
    for blk in blocks:
        subject = bytes.fromhex(blk["s"])
        for name, regexes, flags, multi, ref in harness.block_variants(blk):
            if ref["rc"] != 0:
                continue
            with S.Pool() as pool:
                prog = S.compile(pool, S.parse(pool, regexes, flags, multi))
                got = harness.cli_lines(ENG, prog, subject, ref["ncaps"])
            n += 1
            if got != harness.ref_lines(ref):
                bad.append((blk["file"], blk["name"], name, got, harness.ref_lines(ref)))
    assert n == 3832
    assert not bad, bad[:5]


def test_explicit_expectations_in_the_t_files(lib, blocks):
    """`--- cap` / `--- match_id` / `--- temp_cap` / `--- no_match` sections, e.g.
    t/01-sanity-01.t:112-131, t/04-multi.t:9-121, t/01-sanity-05.t:287-344."""
    n = 0
    for blk in blocks:
        if not ({"cap", "match_id", "temp_cap", "no_match"} & set(blk)):
            continue
        _, regexes, flags, multi, ref = harness.block_variants(blk)[0]
        subject = bytes.fromhex(blk["s"])
        with S.Pool() as pool:
            re = S.parse(pool, regexes, flags, multi)
            prog = S.compile(pool, re)
            lines = harness.cli_lines(ENG, prog, subject, re.ncaps)
        pike, spl = lines[2], lines[3]
        if blk.get("no_match"):
            assert pike == "pike no match"
        if "cap" in blk:
            # the harness strips trailing (-1, -1) groups (t/SRegex.pm:401)
            caps = pike.split(" ", 3)[3] if pike.startswith("pike match") else ""
            while caps.endswith(" (-1, -1)"):
                caps = caps[:-len(" (-1, -1)")]
            assert caps == blk["cap"], (blk["file"], blk["name"], pike)
        if "match_id" in blk:
            assert pike.split()[2] == blk["match_id"], (blk["file"], blk["name"], pike)
        if "temp_cap" in blk:
            body = spl[len("splitted pike "):]
            cut = body.find("match") if "match" in body else body.find("no match")
            assert body[:cut].strip() == blk["temp_cap"].strip(), (blk["file"], blk["name"], spl)
        n += 1
    assert n >= 40


def test_gen_data_streams_match_reference(lib):
    for rec in harness.load_jsonl("gen_data.jsonl"):
        pats = [bytes.fromhex(h) for h in rec["re"]]
        data = S.gen_data_host(rec["n"], bytes.fromhex(rec["tail"]))
        assert len(data) == rec["len"]
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, pats))
            t = ENG.thompson(prog)
            assert t.exec(data, True) == rec["thompson"], rec
            t.close()
            p = ENG.pike(prog, rec["ncaps"])
            rc = p.exec(data, True, want_pending=False)
            assert rc == rec["pike_rc"], rec
            if rc >= 0:
                assert list(p.ovector) == rec["pike_ov"], rec
            p.close()


def test_findall_iteration_matches_reference(lib):
    for rec in harness.load_jsonl("findall.jsonl"):
        pats = [bytes.fromhex(h) for h in rec["re"]]
        data = bytes.fromhex(rec["s"])
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, pats))
            assert harness.findall(ENG, prog, rec["ncaps"], data) == rec["matches"], rec["re"]
            n, spans = ENG.count(prog, data, 2 * (rec["ncaps"] + 1), 1024)
            assert n == len(rec["matches"]) - 1
            assert spans == rec["matches"][:-1]
            assert ENG.final_rc == rec["matches"][-1][0]


# ---------------------------------------------------------------- live vs _ref


def _live_replies(pats, subjects):
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "make_goldens", os.path.join(harness.GOLDEN, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg.live_differential_replies(mg.RefLib(), pats, subjects)


def test_live_differential_against_reference_library(lib):
    """Random subjects over a small alphabet, random chunkings, a pattern zoo
    that leans on assertions, empty matches, nested stars and multi-regex —
    against the real reference library's replies (recorded in
    tests/golden/reference_fuzz.jsonl.gz; the live library in oracle/_ref for
    inputs without a recorded reply)."""
    for pats, subjects in harness.live_differential_cases():
        want = harness.reference_reply(harness.reply_key("live", pats, *subjects),
                                       lambda: _live_replies(pats, subjects), harness.REF_SO)
        ncaps = want["ncaps"]
        assert len(want["runs"]) == len(subjects) == 60, pats
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, pats))
            for data, (findall, thompson) in zip(subjects, want["runs"]):
                assert harness.findall(ENG, prog, ncaps, data) == findall, (pats, data)
                t = ENG.thompson(prog)
                assert t.exec(data, True) == thompson, (pats, data)
                t.close()
