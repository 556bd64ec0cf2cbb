"""The line route by key against the calls a user has without it (sre_hip_route_lines_by_key vs sre_hip_lookup_lines,
sre_hip_route_lines and lookup + download + a numpy sort + upload).

A million 96-byte log lines, each with k=KEY (five letters), the program k=([a-z]+) in mode FIRST on the table-driven
scanner, group [1] (the lines of tools/lookup_probe.py).  A set holds the keys 0 .. S - 1 for S = 1, 200, 4096, 200 000 and
2^20; every line is a member (line i: key i % S, so a slot of 64 lines holds min(S, 64) distinct ids), which takes 1, 1, 2, 3
and 3 digit passes.  Per set size
  (r) the whole route_lines_by_key call (lines, key ids and the bucket table; no index) with the rank rule of a slot the
      library takes by default (one ballot per digit bit), and (t) the same call with SRE_HIP_ROUTE_KEY_RANK=turns (the
      route's wave rule, one ballot per distinct digit of a slot),
  (a) lookup_lines on the same set, which writes the same lines in line order (lines and key ids; no index),
  (b) for the one-pass sizes, route_lines of a four-rule scanner over a million lines of the same length, a quarter to each
      rule (the quarter mix of tools/route_probe.py): the same bytes moved through the route's one 8-bit partition,
  (c) the host tail the call replaces: lookup_lines with index rows, a download of the index and the key ids, a stable sort
      in numpy and an upload of the regrouped index
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after a
warm-up.  A round begins with one untimed lookup_lines call, because the first device call behind the host work of (c) is
slow whichever call it is, and (r) and (t) swap places from round to round.  Then, in a run of its own, the child under rocprofv3 --kernel-trace --stats makes calls (r) and (t); the kernels of
a call are listed per set size and rule with their time and dispatches per call.

--parent-lib PATH: the condition that the calls that existed before cost what they cost before.  lookup_lines, route_lines and
join_lines are timed in child processes that load PATH (a build of the parent commit, through SREGEX_AMD_LIB) and this tree's
library in turn: parent, branch, parent, branch.  A difference between the medians counts as none when it is no larger than
the span of the --reps calls of one parent process; every call's figure is kept.

    python tools/route_key_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile] [--parent-lib PATH --parent-commit ID]
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
from lines_probe import fill_repeat
from lookup_probe import GROUPS, L, NLINES, PATTERN, fill_lines, fill_set, timed, upload
from join_probe import map_rows
from route_probe import block_of, bucket_map, scanners, time_route

SET_SIZES = (1, 200, 4096, 200000, NLINES)
PASSES = {1: 1, 200: 1, 4096: 2, 200000: 3, NLINES: 3}
RULES = ("bits", "turns")
KNOB = "SRE_HIP_ROUTE_KEY_RANK"


def set_rule(rule):
    if rule == "turns":
        os.environ[KNOB] = "turns"
    else:
        os.environ.pop(KNOB, None)


def route_key(sc, buf, nbytes, ks, out, keyid, buckets):
    return sc.route_lines_by_key(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES,
                                 buckets_ptr=buckets.ptr, buckets_cap=NLINES)


def host_tail(sc, buf, nbytes, ks, out, keyid, index, lib):
    """(c): the semi-join on the device, its index and key ids to the host, a stable sort by id, the regrouped index back"""
    info = sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES, index_ptr=index.ptr,
                           index_cap=NLINES)
    idx = np.frombuffer(index.to_bytes(32 * info.nwritten), dtype=np.int64).reshape(-1, 4)
    kid = np.frombuffer(keyid.to_bytes(8 * NLINES), dtype=np.int64)
    order = np.argsort(kid[idx[:, 0]], kind="stable")
    raw = np.ascontiguousarray(idx[order]).tobytes()
    step = 32 << 20
    for o in range(0, len(raw), step):
        assert lib.sre_hip_upload(index.ptr + o, raw[o:o + step], len(raw[o:o + step])) == 0
    return idx[order, 0]


def run_set(lib, pool, prog, multi, size, reps):
    dbuf, dbytes = fill_set(lib, size)
    ks = S.KeySet(dbuf.ptr, dbytes, 1)
    assert (ks.rows, ks.distinct) == (size, size)
    buf, nbytes, nmem = fill_lines(lib, size, 100)
    assert nmem == NLINES and nbytes == NLINES * L
    out, keyid, index, buckets = (S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(40 * NLINES),
                                  S.DeviceBuffer(40 * NLINES))
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    nb = min(size, NLINES)
    want = S.RouteKeyInfo(NLINES, NLINES, NLINES, NLINES, nb, nbytes, NLINES, nbytes)
    one_pass = PASSES[size] == 1
    if one_pass:
        rbuf = fill_repeat(lib, nbytes, block_of("quarter"))
    t = {"bits": [], "turns": [], "lookup": [], "route": [], "host": []}
    outputs = {}
    for rep in range(reps + 1):             # (the first round warms up: code objects, buffers)
        # (c) ends a round with tens of milliseconds of host work, and the first device call behind it takes several
        # times its usual time whichever call it is: an untimed call stands there, and the two rules swap places
        sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES)
        for rule in (RULES if rep % 2 == 0 else RULES[::-1]):
            set_rule(rule)
            d, info = timed(lambda: route_key(sc, buf, nbytes, ks, out, keyid, buckets))
            assert sc.last_lines_device == 1 and info == want, info
            if rep == 0:
                # the first 2 MB and the bucket table: the same with either rule
                outputs[rule] = (out.to_bytes(2 << 20), buckets.to_bytes(40 * min(nb, 1 << 16)))
                idx = sc.route_lines_by_key(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, index_ptr=index.ptr, index_cap=NLINES)
                assert idx == want
                outputs[rule] += (np.frombuffer(index.to_bytes(40 * NLINES), dtype=np.int64).reshape(-1, 5)[:, 0].copy(),)
            elif rep:
                t[rule].append(d)
        set_rule("bits")
        d, linfo = timed(lambda: sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES))
        assert linfo == S.LookupInfo(NLINES, NLINES, NLINES, NLINES, nbytes, NLINES, nbytes), linfo
        if rep:
            t["lookup"].append(d)
        if one_pass:
            d, rinfo, per = time_route(multi, rbuf, nbytes, out, nbytes, bucket_map("quarter"), 5)
            assert rinfo.nwritten == NLINES
            if rep:
                t["route"].append(d)
        d, order = timed(lambda: host_tail(sc, buf, nbytes, ks, out, keyid, index, lib))
        if rep == 0:
            # the device's order is the host's stable sort, line by line, with either rule
            assert (outputs["bits"][2] == order).all() and (outputs["turns"][2] == order).all()
            assert outputs["bits"][:2] == outputs["turns"][:2]
        else:
            t["host"].append(d)
    med = statistics.median
    row = {"set_keys": size, "passes": PASSES[size], "buckets": nb, "lines": NLINES, "bytes": nbytes, "kernel": sc.kernel_name,
           "route_by_key_ms": ms(t["bits"]), "route_by_key_turns_rule_ms": ms(t["turns"]), "lookup_ms": ms(t["lookup"]),
           "route_lines_four_rules_ms": ms(t["route"]) if one_pass else None,
           "host_lookup_download_sort_upload_ms": ms(t["host"]),
           "route_by_key_minus_lookup_ms": (med(t["bits"]) - med(t["lookup"])) * 1e3,
           "route_by_key_over_host_tail": med(t["bits"]) / med(t["host"]),
           "turns_rule_minus_bits_rule_ms": (med(t["turns"]) - med(t["bits"])) * 1e3}
    if one_pass:
        row["route_by_key_minus_route_lines_ms"] = (med(t["bits"]) - med(t["route"])) * 1e3
        rbuf.free()
    for b in (buf, out, keyid, index, buckets, dbuf):
        b.free()
    ks.close()
    return row


def child(calls):
    """the run to put under the profiler: per set size and rule `calls` calls after one warm-up call"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        out, keyid, buckets = S.DeviceBuffer(NLINES * L), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(40 * NLINES)
        for size in SET_SIZES:
            dbuf, dbytes = fill_set(lib, size)
            ks = S.KeySet(dbuf.ptr, dbytes, 1)
            buf, nbytes, _ = fill_lines(lib, size, 100)
            for rule in RULES:
                set_rule(rule)
                for _ in range(calls + 1):
                    route_key(sc, buf, nbytes, ks, out, keyid, buckets)
            for b in (buf, dbuf):
                b.free()
            ks.close()


def short_name(name):
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    return name.split("(")[0]


def profile(calls, stats_out):
    """the child under rocprofv3: per set size and rule the kernels of a call, microseconds and dispatches per call"""
    tmp = tempfile.mkdtemp(prefix="route_key_probe_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--child-calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=500)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert stats and trace, os.listdir(tmp)
        if stats_out:
            shutil.copyfile(stats[0], stats_out)
        with open(trace[0], newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        # a call of the scanner begins with the split's first kernel (so does the creation of a set: its "call" has no
        # kernel of the route by key and is dropped)
        per_call, cur = [], None
        for r in rows:
            name = short_name(r["Kernel_Name"])
            if name.endswith("sre_k_lines_count"):
                cur = {}
                per_call.append(cur)
            if cur is not None:
                us, n = cur.get(name, (0, 0))
                cur[name] = (us + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), n + 1)
        per_call = [c for c in per_call if any("route_key" in n for n in c)]
        configs = [(size, rule) for size in SET_SIZES for rule in RULES]
        assert len(per_call) == len(configs) * (calls + 1), (len(per_call), calls)
        out = []
        for i, (size, rule) in enumerate(configs):
            mine = per_call[i * (calls + 1) + 1:(i + 1) * (calls + 1)]
            names = sorted({n for c in mine for n in c})
            kernels = {n: {"us": statistics.median([c.get(n, (0, 0))[0] for c in mine]) / 1e3, "dispatches": mine[0].get(n, (0, 0))[1]}
                       for n in names}
            part = sum(v["us"] for n, v in kernels.items() if "partition_count" in n or "partition_scatter" in n)
            out.append({"set_keys": size, "passes": PASSES[size], "rule": rule, "kernels": kernels,
                        "count_and_scatter_us": part, "count_and_scatter_us_per_pass": part / PASSES[size],
                        "all_kernels_us": statistics.median([sum(v[0] for v in c.values()) for c in mine]) / 1e3})
        with open(stats[0], newline="") as f:
            top = stats_top(csv.DictReader(f), 24)
        return out, top
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def older(reps):
    """lookup_lines, route_lines and join_lines with whatever library this process loaded"""
    lib = S.load_library()
    size, nbytes = 4096, NLINES * L
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        multi, _ = scanners(pool)
        dbuf, dbytes = fill_set(lib, size)
        ks = S.KeySet(dbuf.ptr, dbytes, 1)
        mbuf, mbytes = upload(lib, map_rows(size, 1).tobytes())
        km = S.KeySet(mbuf.ptr, mbytes, 2, nkeys=1)
        buf, _, _ = fill_lines(lib, size, 100)
        rbuf = fill_repeat(lib, nbytes, block_of("quarter"))
        out, keyid = S.DeviceBuffer(NLINES * (L + 9)), S.DeviceBuffer(8 * NLINES)
        tl, tr, tj = [], [], []
        for rep in range(reps + 1):
            d, info = timed(lambda: sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES))
            assert info.nwritten == NLINES
            tl.append(d)
            d, rinfo, _ = time_route(multi, rbuf, nbytes, out, nbytes, bucket_map("quarter"), 5)
            assert rinfo.nwritten == NLINES
            tr.append(d)
            d, jinfo = timed(lambda: sc.join_lines(buf.ptr, nbytes, out.ptr, NLINES * (L + 9), GROUPS, km, [0], keyid_ptr=keyid.ptr,
                                                   keyid_cap=NLINES))
            assert jinfo.nwritten == NLINES
            tj.append(d)
        print(json.dumps({"lookup_ms": ms(tl[1:]), "route_lines_ms": ms(tr[1:]), "join_ms": ms(tj[1:])}))


def older_ab(parent_lib, reps):
    """parent, branch, parent, branch in child processes of their own; per call the runs and whether the branch's medians
    lie inside the spread of all the parent's runs"""
    runs = []
    for which in ("parent", "branch", "parent", "branch"):
        env = dict(os.environ)
        env.pop("SREGEX_AMD_LIB", None)
        env.pop(KNOB, None)
        if which == "parent":
            env["SREGEX_AMD_LIB"] = parent_lib
        text = subprocess.run([sys.executable, os.path.abspath(__file__), "--older", "--reps", str(reps)], check=True, env=env,
                              stdout=subprocess.PIPE, timeout=300).stdout.decode()
        runs.append((which, json.loads(text.strip().splitlines()[-1])))
    rows = []
    for metric in ("lookup_ms", "route_lines_ms", "join_ms"):
        p_runs = [r[metric]["all"] for w, r in runs if w == "parent"]
        p = [r[metric]["median"] for w, r in runs if w == "parent"]
        b = [r[metric]["median"] for w, r in runs if w == "branch"]
        # the spread of the parent's own runs: the widest span of the `reps` calls of one parent process
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
    doc = {"tool": "tools/route_key_probe.py", "parent_commit": args.parent_commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps after a warm-up; route_lines_by_key with either rank "
                     "rule (lines, key ids, bucket table), lookup_lines on the same set (lines and key ids), route_lines of four "
                     "rules over as many lines (one-pass sizes) and lookup_lines with index + download of index and key ids + a "
                     "stable numpy sort + upload alternating in one process; every line is a member, line i has key i % set_keys",
           "pattern": PATTERN.decode(), "groups": GROUPS, "results": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        multi, _ = scanners(pool)
        for size in SET_SIZES:
            r = run_set(lib, pool, prog, multi, size, args.reps)
            print(json.dumps(r), flush=True)
            doc["results"].append(r)
    by = {r["set_keys"]: r["route_by_key_ms"]["median"] for r in doc["results"]}
    doc["ms_per_added_pass"] = {"from": "(3 passes at 2^20 keys - 1 pass at 200 keys) / 2, whole calls; the kernels' own times are "
                                        "under `kernels`", "value": (by[NLINES] - by[200]) / 2}
    if not args.no_profile:
        per, top = profile(3, args.stats_out)
        doc["kernels"] = {"run": "route_lines_by_key with either rank rule under rocprofv3 --kernel-trace --stats, in a run of its "
                                 "own: 3 calls per set size and rule after a warm-up call, whose dispatches are left out; median "
                                 "microseconds per call and kernel, and the dispatches of a call",
                          "kernel_stats_top": top, "rows": per}
    if args.parent_lib:
        doc["older_calls_parent_vs_branch"] = {
            "run": "lookup_lines (4096 keys), route_lines (four rules, a quarter each) and join_lines (4096 keys, one column) over a "
                   "million lines in child processes that load the parent commit's library and this tree's in turn (parent, branch, "
                   "parent, branch); medians of reps after a warm-up",
            "rows": older_ab(args.parent_lib, args.reps)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
