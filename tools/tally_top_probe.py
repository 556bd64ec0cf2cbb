"""The ordered tally against the calls a user has without it (sre_hip_tally_top_lines vs sre_hip_tally_sums_lines and
tally_sums_lines + download + a numpy sort + take).

A million 96-byte log lines, each with k=KEY (five letters) and v=NUMBER (18 digits, zero-padded), the program
k=([a-z]+) v=([0-9]+) in mode FIRST on the table-driven scanner, key group 1, value group 2; line i has key i % keys, so a
buffer holds exactly 1, 4096, 200 000 or 2^20 distinct keys.  Per key count
  (t) the whole tally_top_lines call (rows, counts, aggregates; no ranks, no index), by COUNT and by SUM, descending, with
      limit 0 and limit 100,
  (a) tally_sums_lines on the same buffer with the same arrays: the same tally, no order,
  (b) the host alternative the call replaces: tally_sums_lines, a download of counts, sums and rows, a stable numpy argsort
      and a take of the three on the host
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after a
warm-up.  Then, in a run of its own, the child under rocprofv3 --kernel-trace --stats makes the calls (t) by SUM with limit 0;
the kernels of a call are listed per key count with their time and dispatches per call.

--parent-lib PATH: the condition that the calls that existed before cost what they cost before.  tally_lines,
tally_sums_lines and sort_lines are timed in child processes that load PATH (a build of the parent commit, through
SREGEX_AMD_LIB) and this tree's library in turn: parent, parent, branch, parent, branch; so is tally_top_lines, by COUNT and by
SUM, descending, limit 0, at 4096 and 200 000 keys, which the parent has too.  The first two parent runs are the
A/A pair: their difference is the noise of the box.  A difference between the medians of branch and parent counts as none
when it is no larger than the A/A difference or the span of the --reps calls of one parent process.

    python tools/tally_top_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile] [--parent-lib PATH --parent-commit ID]
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
from lookup_probe import L, NLINES, WIDTH, timed
from sort_probe import PATTERN, fill_lines, short_name, sort_call

KEY_GROUP, VALUE_GROUP = [1], [2]
SPAN = 1 << 24
KEYS = (1, 4096, 200000, NLINES)
LIMITS = (0, 100)
BYS = {"count": S.HIP_TOP_COUNT, "sum": S.HIP_TOP_SUM}
NEW_KERNELS = ("sre_k_tally_top_first", "sre_k_values_init", "sre_k_values<TopVals>", "sre_k_tally_top_table",
               "sre_k_tally_top_permute", "sre_k_tally_top_ranks")
OLDER_TOP_KEYS = (4096, 200000)


def top_call(sc, buf, nbytes, out, counts, sums, by, limit, rank=None):
    return sc.tally_top_lines(buf.ptr, nbytes, out.ptr, nbytes, KEY_GROUP, VALUE_GROUP, NLINES, by=by, descending=True, limit=limit,
                              counts_ptr=counts.ptr, counts_cap=NLINES, sums_ptr=sums.ptr, sums_cap=NLINES,
                              rank_ptr=rank.ptr if rank else None, rank_cap=NLINES if rank else 0)


def sums_call(sc, buf, nbytes, out, counts, sums):
    return sc.tally_sums_lines(buf.ptr, nbytes, out.ptr, nbytes, KEY_GROUP, VALUE_GROUP, NLINES, counts_ptr=counts.ptr, counts_cap=NLINES,
                               sums_ptr=sums.ptr, sums_cap=NLINES)


def host_alternative(sc, buf, nbytes, out, counts, sums, by, limit):
    """(b): the tally on the device, its three arrays to the host, a stable argsort there and the take"""
    info = sums_call(sc, buf, nbytes, out, counts, sums)
    c = np.frombuffer(counts.to_bytes(8 * info.nkeys), dtype=np.uint64)
    s = np.frombuffer(sums.to_bytes(32 * info.nkeys), dtype=np.int64).reshape(-1, 4)
    rows = np.frombuffer(out.to_bytes(info.out_bytes), dtype=np.uint8).reshape(-1, WIDTH + 1)
    v = c.astype(np.int64) if by == S.HIP_TOP_COUNT else s[:, 0]
    order = np.argsort(-v, kind="stable")
    if limit:
        order = order[:limit]
    return c[order], s[order], rows[order]


def run_keys(lib, pool, prog, keys, reps):
    buf, nbytes, _ = fill_lines(lib, SPAN, keys)
    assert nbytes == NLINES * L
    out, counts, sums = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(32 * NLINES)
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    configs = [(name, limit) for name in BYS for limit in LIMITS]
    t = {c: [] for c in configs}
    t.update({("host",) + c: [] for c in configs})
    t["sums"] = []
    passes = {}
    for rep in range(reps + 1):             # (the first round warms up: code objects, buffers)
        sc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes)
        for name, limit in (configs if rep % 2 == 0 else configs[::-1]):
            d, info = timed(lambda: top_call(sc, buf, nbytes, out, counts, sums, BYS[name], limit))
            nrows = min(limit, keys) if limit else keys
            assert sc.last_lines_device == 1 and (info.nlines, info.nselected, info.nkeys, info.nordered, info.nrows, info.nwritten) == \
                (NLINES, NLINES, keys, keys, nrows, nrows), info
            passes[name] = info.passes
            if rep == 0:
                # the device's order is the host's stable sort, row by row
                got = (np.frombuffer(counts.to_bytes(8 * nrows), dtype=np.uint64).copy(),
                       np.frombuffer(sums.to_bytes(32 * nrows), dtype=np.int64).reshape(-1, 4).copy(),
                       np.frombuffer(out.to_bytes(info.out_bytes), dtype=np.uint8).reshape(-1, WIDTH + 1).copy())
                want = host_alternative(sc, buf, nbytes, out, counts, sums, BYS[name], limit)
                assert all((g == w).all() for g, w in zip(got, want)), (keys, name, limit)
            else:
                t[(name, limit)].append(d)
        d, sinfo = timed(lambda: sums_call(sc, buf, nbytes, out, counts, sums))
        assert sinfo.nkeys == keys
        if rep:
            t["sums"].append(d)
        for name, limit in configs:
            d, _ = timed(lambda: host_alternative(sc, buf, nbytes, out, counts, sums, BYS[name], limit))
            if rep:
                t[("host", name, limit)].append(d)
    med = statistics.median
    row = {"keys": keys, "lines": NLINES, "bytes": nbytes, "kernel": sc.kernel_name, "passes": passes,
           "tally_top_ms": {"%s_limit_%d" % c: ms(t[c]) for c in configs},
           "tally_sums_lines_ms": ms(t["sums"]),
           "host_tally_download_argsort_take_ms": {"%s_limit_%d" % c: ms(t[("host",) + c]) for c in configs},
           "top_minus_tally_sums_ms": {"%s_limit_%d" % c: (med(t[c]) - med(t["sums"])) * 1e3 for c in configs},
           "top_over_host_alternative": {"%s_limit_%d" % c: med(t[c]) / med(t[("host",) + c]) for c in configs}}
    row["top_faster_than_host_alternative"] = all(med(t[c]) < med(t[("host",) + c]) for c in configs)
    for b in (buf, out, counts, sums):
        b.free()
    return row


def child(calls):
    """the run to put under the profiler: per key count `calls` calls by SUM with limit 0 after one warm-up call"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        out, counts, sums, rank = (S.DeviceBuffer(NLINES * L), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(32 * NLINES),
                                   S.DeviceBuffer(8 * NLINES))
        for keys in KEYS:
            buf, nbytes, _ = fill_lines(lib, SPAN, keys)
            for _ in range(calls + 1):
                top_call(sc, buf, nbytes, out, counts, sums, S.HIP_TOP_SUM, 0, rank)
            buf.free()


def profile(calls, stats_out):
    """the child under rocprofv3: per key count the kernels of a call, microseconds and dispatches per call"""
    tmp = tempfile.mkdtemp(prefix="tally_top_probe_")
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
        per_call, cur = [], None
        for r in rows:
            name = short_name(r["Kernel_Name"])
            if name.endswith("sre_k_lines_count"):      # (a call of the scanner begins with the split's first kernel)
                cur = {}
                per_call.append(cur)
            if cur is not None:
                us, n = cur.get(name, (0, 0))
                cur[name] = (us + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), n + 1)
        per_call = [c for c in per_call if any("k_tally_top_" in n for n in c)]
        assert len(per_call) == len(KEYS) * (calls + 1), (len(per_call), calls)
        out = []
        for i, keys in enumerate(KEYS):
            mine = per_call[i * (calls + 1) + 1:(i + 1) * (calls + 1)]
            names = sorted({n for c in mine for n in c})
            kernels = {n: {"us": statistics.median([c.get(n, (0, 0))[0] for c in mine]) / 1e3, "dispatches": mine[0].get(n, (0, 0))[1]}
                       for n in names}
            part = [v for n, v in kernels.items() if "partition_count" in n or "partition_scatter" in n]
            npass = max(1, sum(v["dispatches"] for n, v in kernels.items() if "partition_count" in n))
            out.append({"keys": keys, "call": "tally_top_lines by SUM, descending, limit 0, with ranks", "kernels": kernels,
                        "new_kernels_us": sum(v["us"] for n, v in kernels.items() if any(n.endswith(k) for k in NEW_KERNELS)),
                        "digit_passes": npass, "count_and_scatter_us_per_pass": sum(v["us"] for v in part) / npass,
                        "all_kernels_us": statistics.median([sum(v[0] for v in c.values()) for c in mine]) / 1e3})
        with open(stats[0], newline="") as f:
            top = stats_top(csv.DictReader(f), 24)
        return out, top
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def older_metrics():
    return ["tally_lines_ms", "tally_sums_lines_ms", "sort_lines_ms"] + \
        ["tally_top_lines_%s_%d_keys_ms" % (name, keys) for keys in OLDER_TOP_KEYS for name in BYS]


def older(reps):
    """tally_lines, tally_sums_lines and sort_lines (4096 keys), and tally_top_lines by COUNT and by SUM, descending, limit 0, at
    4096 and 200 000 keys, with whatever library this process loaded"""
    lib = S.load_library()
    size = 4096
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        buf, nbytes, _ = fill_lines(lib, SPAN, size)
        out, counts, sums = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(32 * NLINES)
        tt, ts, to = [], [], []
        for rep in range(reps + 1):
            d, info = timed(lambda: sc.tally_lines(buf.ptr, nbytes, out.ptr, nbytes, KEY_GROUP, NLINES, counts_ptr=counts.ptr,
                                                   counts_cap=NLINES))
            assert info.nkeys == size
            tt.append(d)
            d, info = timed(lambda: sums_call(sc, buf, nbytes, out, counts, sums))
            assert info.nkeys == size
            ts.append(d)
            d, sinfo = timed(lambda: sort_call(sc, buf, nbytes, out, False, 0))
            assert sinfo.nwritten == NLINES and sinfo.passes == 3
            to.append(d)
        res = {"tally_lines_ms": ms(tt[1:]), "tally_sums_lines_ms": ms(ts[1:]), "sort_lines_ms": ms(to[1:])}
        for keys in OLDER_TOP_KEYS:
            if keys != size:
                buf.free()
                buf, nbytes, _ = fill_lines(lib, SPAN, keys)
            for name in BYS:
                tp = []
                for rep in range(reps + 1):
                    d, info = timed(lambda: top_call(sc, buf, nbytes, out, counts, sums, BYS[name], 0))
                    assert (info.nkeys, info.nrows, info.nwritten) == (keys, keys, keys), info
                    tp.append(d)
                res["tally_top_lines_%s_%d_keys_ms" % (name, keys)] = ms(tp[1:])
        print(json.dumps(res))


def older_ab(parent_lib, reps):
    """parent, parent, branch, parent, branch in child processes of their own; per call the runs, the A/A difference of the first
    two parent runs and whether the branch's medians lie inside the noise"""
    runs = []
    for which in ("parent", "parent", "branch", "parent", "branch"):
        env = dict(os.environ)
        env.pop("SREGEX_AMD_LIB", None)
        if which == "parent":
            env["SREGEX_AMD_LIB"] = parent_lib
        text = subprocess.run([sys.executable, os.path.abspath(__file__), "--older", "--reps", str(reps)], check=True, env=env,
                              stdout=subprocess.PIPE, timeout=300).stdout.decode()
        runs.append((which, json.loads(text.strip().splitlines()[-1])))
    rows = []
    for metric in older_metrics():
        p_runs = [r[metric]["all"] for w, r in runs if w == "parent"]
        p = [r[metric]["median"] for w, r in runs if w == "parent"]
        b = [r[metric]["median"] for w, r in runs if w == "branch"]
        spread = max(max(x) - min(x) for x in p_runs)
        aa = abs(p[0] - p[1])
        diff = statistics.median(b) - statistics.median(p)
        rows.append({"metric": metric, "parent_medians_ms": p, "branch_medians_ms": b, "parent_runs_ms": p_runs,
                     "branch_runs_ms": [r[metric]["all"] for w, r in runs if w == "branch"],
                     "parent_a_a_difference_ms": aa, "branch_minus_parent_ms": diff, "parent_spread_ms": spread,
                     "difference_within_noise": abs(diff) <= max(spread, aa)})
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
    doc = {"tool": "tools/tally_top_probe.py", "parent_commit": args.parent_commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps after a warm-up; tally_top_lines (rows, counts, "
                     "aggregates; no ranks, no index) by COUNT and by SUM, descending, with limit 0 and 100, tally_sums_lines on the "
                     "same buffer, and tally_sums_lines + download of counts, sums and rows + a stable numpy argsort + take "
                     "alternating in one process; line i has key i % keys and an 18-digit number below 2^24",
           "pattern": PATTERN.decode(), "key_group": KEY_GROUP, "value_group": VALUE_GROUP, "results": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        for keys in KEYS:
            r = run_keys(lib, pool, prog, keys, args.reps)
            print(json.dumps(r), flush=True)
            doc["results"].append(r)
    doc["top_faster_than_host_alternative_at_every_key_count"] = all(r["top_faster_than_host_alternative"] for r in doc["results"])
    if not args.no_profile:
        per, top = profile(3, args.stats_out)
        doc["kernels"] = {"run": "tally_top_lines by SUM, descending, limit 0, with ranks, under rocprofv3 --kernel-trace --stats, in a "
                                 "run of its own: 3 calls per key count after a warm-up call, whose dispatches are left out; median "
                                 "microseconds per call and kernel, and the dispatches of a call",
                          "kernel_stats_top": top, "rows": per}
    if args.parent_lib:
        doc["older_calls_parent_vs_branch"] = {
            "run": "tally_lines, tally_sums_lines (4096 keys, one value column), sort_lines (ascending, no limit, 2^24 values: three "
                   "passes) and tally_top_lines (by COUNT and by SUM, descending, limit 0, 4096 and 200 000 keys) over a million lines in "
                   "child processes that load the parent commit's library and this tree's in turn "
                   "(parent, parent, branch, parent, branch); medians of reps after a warm-up; the first two parent runs are the A/A pair",
            "rows": older_ab(args.parent_lib, args.reps)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
