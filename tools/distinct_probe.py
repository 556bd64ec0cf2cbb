"""The line distinct against the calls a user has without it (sre_hip_distinct_lines vs sre_hip_lookup_lines,
sre_hip_filter_lines and tally + download + numpy + upload + a second call).

A million 96-byte log lines, each with k=KEY (five letters) and a mark, the program k=([a-z]+) in mode FIRST on the
table-driven scanner, group [1] (the lines of tools/lookup_probe.py).  Line i carries key i % D for D = 1, 4096, 200 000 and
2^20 distinct keys, so a key's lines are D apart, its first line is one of the first D lines and its last one of the last D;
the mark is m=1 on the first D lines and m=0 elsewhere.  Per D
  (f) distinct_lines FIRST, 1, 0 (the first D lines), (l) LAST, 1, 0 (the last D lines) and (e) EVERY, 2, 0 (every line,
      none at D = 2^20), each with both per-line arrays and no index,
  (a) lookup_lines of a scanner for m=([01]) against the set {"1"}, and (b) filter_lines of a scanner for m=1: both write the
      lines FIRST writes, with no table of the buffer's keys at all; (c) filter_lines of the key scanner, which writes the
      lines EVERY writes below D = 2^20,
  (t) tally_lines of the same group (rows, counts and key ids), which runs the same insert, and
  (h) the host alternative to FIRST: tally_lines, a download of its key ids and counts, the first line of every key by numpy,
      an upload of a byte per line, and a second call that writes as many lines (the library has no call that takes a
      per-line mask: the second call is (b))
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after a
warm-up.  Then, in a run of its own, the child under rocprofv3 --kernel-trace --stats makes calls (f), (l) and (e); the
kernels of a call are listed per D and rule with their time and dispatches per call.

--parent-lib PATH: the condition that the calls that existed before cost what they cost before.  tally_lines, lookup_lines
and filter_lines are timed in child processes that load PATH (a build of the parent commit, through SREGEX_AMD_LIB) and this
tree's library in turn: parent, branch, parent, branch.

    python tools/distinct_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile] [--parent-lib PATH --parent-commit ID]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sregex_amd as S
from filter_probe import ms
from extract_probe import stats_top
from lookup_probe import GROUPS, HEAD, L, NLINES, PATTERN, WIDTH, key_columns, timed, upload

KEYS = (1, 4096, 200000, NLINES)
MARK, MARK_GROUP = rb"m=1", rb"m=([01])"
RULES = (("first", 0, 1), ("last", 1, 1), ("every", 2, 2))        # name, which, min_count


def fill_lines(lib, nkeys):
    """the buffer: line i = HEAD, the key i % nkeys, the mark (1 on the first nkeys lines), a tail of x, a newline"""
    row = np.frombuffer((HEAD + b"a" * WIDTH + b" m=0 user nobody " + b"x" * L)[:L - 1] + b"\n", dtype=np.uint8)
    a = np.tile(row, (NLINES, 1))
    i = np.arange(NLINES, dtype=np.int64)
    for j, col in enumerate(key_columns(i % nkeys)):
        a[:, len(HEAD) + j] = col
    a[:, len(HEAD) + WIDTH + 3] = np.where(i < nkeys, ord("1"), ord("0"))
    return upload(lib, a.tobytes())


def distinct(sc, buf, nbytes, out, kc, kl, which, lo):
    return sc.distinct_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, NLINES, which, lo, 0, keycount_ptr=kc.ptr, keycount_cap=NLINES,
                             keyline_ptr=kl.ptr, keyline_cap=NLINES)


def want_info(nkeys, which, lo):
    per = NLINES // nkeys           # (every key has per or per + 1 lines)
    kept = nkeys if per >= lo else 0
    nsel = (NLINES if which == 2 else nkeys) if kept else 0
    return S.DistinctInfo(NLINES, NLINES, nkeys, kept, nsel, nsel * L, nsel, nsel * L)


def host_alternative(lib, sc, fsc, buf, nbytes, out, keyid, counts, mask):
    """(h): the tally on the device, its key ids and counts to the host, the first line of every key by numpy, a byte per
    line back, and a second call that writes the lines"""
    info = sc.tally_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, NLINES, counts_ptr=counts.ptr, counts_cap=NLINES,
                          keyid_ptr=keyid.ptr, keyid_cap=NLINES)
    kid = np.frombuffer(keyid.to_bytes(8 * NLINES), dtype=np.int64)
    cnt = np.frombuffer(counts.to_bytes(8 * info.nkeys), dtype=np.uint64)
    _, first = np.unique(kid, return_index=True)
    sel = np.zeros(NLINES, dtype=np.uint8)
    sel[first[cnt[kid[first]] >= 1]] = 1
    raw = sel.tobytes()
    assert lib.sre_hip_upload(mask.ptr, raw, len(raw)) == 0
    second = fsc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes)
    return int(sel.sum()), second.nwritten


def run_keys(lib, pool, progs, nkeys, reps):
    prog, mark, mgroup = progs
    buf, nbytes = fill_lines(lib, nkeys)
    out, kc, kl, keyid, counts, mask = (S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(8 * NLINES),
                                        S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(NLINES))
    one, _ = upload(lib, b"1\n")
    ks = S.KeySet(one.ptr, 2, 1)
    sc, fsc, lsc = (S.Scanner(pool, p, S.HIP_PIKE_FIRST) for p in (prog, mark, mgroup))
    assert sc.engine == S.ENGINE_SCAN
    t = {k: [] for k in ("first", "last", "every", "lookup", "filter_mark", "filter_all", "tally", "host")}
    for rep in range(reps + 1):             # (the first round warms up: code objects, buffers)
        # (h) ends a round with host work, and the first device call behind it is slow whichever call it is: an untimed call
        sc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes)
        order = RULES if rep % 2 == 0 else RULES[::-1]
        for name, which, lo in order:
            d, info = timed(lambda: distinct(sc, buf, nbytes, out, kc, kl, which, lo))
            assert sc.last_lines_device == 1 and info == want_info(nkeys, which, lo), (name, info)
            if rep == 0 and name != "every":
                # the lines are the first (the last) nkeys lines of the buffer, and a key's first line is line % nkeys
                head = out.to_bytes(min(info.out_bytes, 1 << 20))
                at = 0 if name == "first" else (NLINES - nkeys) * L
                assert head == buf.to_bytes(at + len(head))[at:]
                line = np.frombuffer(kl.to_bytes(8 * NLINES), dtype=np.int64)
                assert (line == np.arange(NLINES) % nkeys).all()
            elif rep:
                t[name].append(d)
        d, linfo = timed(lambda: lsc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES))
        assert linfo.nwritten == nkeys, linfo
        df, finfo = timed(lambda: fsc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes))
        assert finfo.nwritten == nkeys, finfo
        da, ainfo = timed(lambda: sc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes))
        assert ainfo.nwritten == NLINES
        dt, tinfo = timed(lambda: sc.tally_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, NLINES, counts_ptr=counts.ptr, counts_cap=NLINES,
                                                 keyid_ptr=keyid.ptr, keyid_cap=NLINES))
        assert tinfo.nkeys == nkeys
        dh, (nsel, nsecond) = timed(lambda: host_alternative(lib, sc, fsc, buf, nbytes, out, keyid, counts, mask))
        assert nsel == nsecond == nkeys
        if rep:
            for k, v in (("lookup", d), ("filter_mark", df), ("filter_all", da), ("tally", dt), ("host", dh)):
                t[k].append(v)
    med = statistics.median
    row = {"distinct_keys": nkeys, "lines": NLINES, "bytes": nbytes, "kernel": sc.kernel_name,
           "distinct_first_ms": ms(t["first"]), "distinct_last_ms": ms(t["last"]), "distinct_every_min2_ms": ms(t["every"]),
           "lookup_same_lines_as_first_ms": ms(t["lookup"]), "filter_same_lines_as_first_ms": ms(t["filter_mark"]),
           "filter_every_line_ms": ms(t["filter_all"]), "tally_ms": ms(t["tally"]),
           "host_tally_download_numpy_upload_second_call_ms": ms(t["host"]),
           "first_minus_lookup_ms": (med(t["first"]) - med(t["lookup"])) * 1e3,
           "last_minus_first_ms": (med(t["last"]) - med(t["first"])) * 1e3,
           "first_minus_tally_ms": (med(t["first"]) - med(t["tally"])) * 1e3,
           "first_over_host_alternative": med(t["first"]) / med(t["host"])}
    for b in (buf, out, kc, kl, keyid, counts, mask, one):
        b.free()
    ks.close()
    return row


def child(calls):
    """the run to put under the profiler: per D and rule `calls` calls after one warm-up call"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        out, kc, kl = S.DeviceBuffer(NLINES * L), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(8 * NLINES)
        for nkeys in KEYS:
            buf, nbytes = fill_lines(lib, nkeys)
            for _, which, lo in RULES:
                for _ in range(calls + 1):
                    distinct(sc, buf, nbytes, out, kc, kl, which, lo)
            buf.free()


def short_name(name):
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    return name.split("(")[0]


def profile(calls, stats_out):
    """the child under rocprofv3: per D and rule the kernels of a call, microseconds and dispatches per call"""
    tmp = tempfile.mkdtemp(prefix="distinct_probe_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--child-calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=400)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert stats and trace, os.listdir(tmp)
        if stats_out:
            shutil.copyfile(stats[0], stats_out)
        with open(trace[0], newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        # a call of the scanner begins with the split's first kernel
        per_call, cur = [], None
        for r in rows:
            name = short_name(r["Kernel_Name"])
            if name.endswith("sre_k_lines_count"):
                cur = {}
                per_call.append(cur)
            if cur is not None:
                us, n = cur.get(name, (0, 0))
                cur[name] = (us + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), n + 1)
        configs = [(nkeys, name) for nkeys in KEYS for name, _, _ in RULES]
        assert len(per_call) == len(configs) * (calls + 1), (len(per_call), calls)
        out = []
        for i, (nkeys, rule) in enumerate(configs):
            mine = per_call[i * (calls + 1) + 1:(i + 1) * (calls + 1)]
            names = sorted({n for c in mine for n in c})
            kernels = {n: {"us": statistics.median([c.get(n, (0, 0))[0] for c in mine]) / 1e3, "dispatches": mine[0].get(n, (0, 0))[1]}
                       for n in names}
            own = sum(v["us"] for n, v in kernels.items() if "distinct" in n)
            out.append({"distinct_keys": nkeys, "rule": rule, "kernels": kernels, "distinct_kernels_us": own,
                        "tally_insert_and_keep_us": sum(v["us"] for n, v in kernels.items() if "tally" in n),
                        "all_kernels_us": statistics.median([sum(v[0] for v in c.values()) for c in mine]) / 1e3})
        with open(stats[0], newline="") as f:
            top = stats_top(csv.DictReader(f), 24)
        return out, top
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def older(reps):
    """tally_lines, lookup_lines and filter_lines with whatever library this process loaded"""
    lib = S.load_library()
    nkeys = 4096
    with S.Pool() as pool:
        prog, mark, mgroup = (S.compile(pool, S.parse(pool, [p])) for p in (PATTERN, MARK, MARK_GROUP))
        sc, fsc, lsc = (S.Scanner(pool, p, S.HIP_PIKE_FIRST) for p in (prog, mark, mgroup))
        buf, nbytes = fill_lines(lib, nkeys)
        one, _ = upload(lib, b"1\n")
        ks = S.KeySet(one.ptr, 2, 1)
        out, keyid, counts = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(8 * NLINES)
        tt, tl, tf = [], [], []
        for rep in range(reps + 1):
            d, info = timed(lambda: sc.tally_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, NLINES, counts_ptr=counts.ptr,
                                                   counts_cap=NLINES, keyid_ptr=keyid.ptr, keyid_cap=NLINES))
            assert info.nkeys == nkeys
            tt.append(d)
            d, info = timed(lambda: lsc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES))
            assert info.nwritten == nkeys
            tl.append(d)
            d, info = timed(lambda: fsc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes))
            assert info.nwritten == nkeys
            tf.append(d)
        print(json.dumps({"tally_ms": ms(tt[1:]), "lookup_ms": ms(tl[1:]), "filter_ms": ms(tf[1:])}))


def older_ab(parent_lib, reps):
    """parent, branch, parent, branch in child processes of their own; per call the runs and whether the branch's medians
    lie inside the spread of the parent's runs"""
    runs = []
    for which in ("parent", "branch", "parent", "branch"):
        env = dict(os.environ)
        env.pop("SREGEX_AMD_LIB", None)
        if which == "parent":
            env["SREGEX_AMD_LIB"] = parent_lib
        text = subprocess.run([sys.executable, os.path.abspath(__file__), "--older", "--reps", str(reps)], check=True, env=env,
                              stdout=subprocess.PIPE, timeout=300).stdout.decode()
        runs.append((which, json.loads(text.strip().splitlines()[-1])))
    rows = []
    for metric in ("tally_ms", "lookup_ms", "filter_ms"):
        p_runs = [r[metric]["all"] for w, r in runs if w == "parent"]
        p = [r[metric]["median"] for w, r in runs if w == "parent"]
        b = [r[metric]["median"] for w, r in runs if w == "branch"]
        spread = max(max(x) - min(x) for x in p_runs)
        diff = statistics.median(b) - statistics.median(p)
        rows.append({"metric": metric, "parent_medians_ms": p, "branch_medians_ms": b, "parent_runs_ms": p_runs,
                     "branch_runs_ms": [r[metric]["all"] for w, r in runs if w == "branch"],
                     "branch_minus_parent_ms": diff, "parent_spread_ms": spread,
                     "difference_within_parent_spread": abs(diff) <= spread})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-out", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default=None, help="the commit --parent-lib was built from, for the record")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-calls", type=int, default=3, help=argparse.SUPPRESS)
    ap.add_argument("--older", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child_calls)
        return
    if args.older:
        older(args.reps)
        return
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    doc = {"tool": "tools/distinct_probe.py", "parent_commit": args.parent_commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps after a warm-up; distinct_lines FIRST, LAST and EVERY "
                     "with min_count 2 (lines and both per-line arrays), lookup_lines and filter_lines that write FIRST's lines, "
                     "filter_lines of every line, tally_lines (rows, counts, key ids) and tally + download + numpy + upload + a "
                     "second call alternating in one process; line i has key i % distinct_keys",
           "pattern": PATTERN.decode(), "groups": GROUPS, "results": []}
    with S.Pool() as pool:
        progs = [S.compile(pool, S.parse(pool, [p])) for p in (PATTERN, MARK, MARK_GROUP)]
        for nkeys in KEYS:
            r = run_keys(lib, pool, progs, nkeys, args.reps)
            print(json.dumps(r), flush=True)
            doc["results"].append(r)
    if not args.no_profile:
        per, top = profile(3, args.stats_out)
        doc["kernels"] = {"run": "distinct_lines FIRST, LAST and EVERY under rocprofv3 --kernel-trace --stats, in a run of its own: 3 "
                                 "calls per number of keys and rule after a warm-up call, whose dispatches are left out; median "
                                 "microseconds per call and kernel, and the dispatches of a call",
                          "kernel_stats_top": top, "rows": per}
    if args.parent_lib:
        doc["older_calls_parent_vs_branch"] = {
            "run": "tally_lines, lookup_lines and filter_lines over a million lines of 4096 keys in child processes that load the "
                   "parent commit's library and this tree's in turn (parent, branch, parent, branch); medians of reps after a warm-up",
            "rows": older_ab(args.parent_lib, args.reps)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
