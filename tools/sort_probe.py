"""The line sort against the calls a user has without it (sre_hip_sort_lines vs sre_hip_filter_lines,
sre_hip_route_lines_by_key and extract + download + a numpy sort + upload).

A million 96-byte log lines, each with k=KEY (five letters) and v=NUMBER (18 digits, zero-padded), the program
k=([a-z]+) v=([0-9]+) in mode FIRST on the table-driven scanner, sort group 2.  The numbers of a buffer are spread by a
multiplicative hash over a range that takes 1, 3, 4 or 8 digit passes (256, 2^24, 2^32, 10^18 values).  Per range
  (s) the whole sort_lines call (the lines; no index), ascending and descending, with limit 0 and limit 100,
  (a) filter_lines on the same buffer, which writes the same lines in line order: the same bytes moved, no sort,
  (b) for 1 and 3 passes, route_lines_by_key on the same lines by group 1 with a set of 200 resp. 200 000 keys (line i has
      key i % size: every line is a member), which takes as many passes with one-word items,
  (c) the host tail the call replaces: extract_lines of the number, a download of the rows, a stable argsort in numpy and
      an upload of the permutation
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after a
warm-up.  A round begins with one untimed filter_lines call, because the first device call behind the host work of (c) is
slow whichever call it is.  Then, in a run of its own, the child under rocprofv3 --kernel-trace --stats makes the calls
(s) ascending with limit 0 and (b); the kernels of a call are listed per range with their time and dispatches per call.

--parent-lib PATH: the condition that the calls that existed before cost what they cost before.  lookup_lines,
route_lines_by_key, tally_sums_lines and sort_lines (three passes) are timed in child processes that load PATH (a build of the parent commit, through
SREGEX_AMD_LIB) and this tree's library in turn: parent, branch, parent, branch.  A difference between the medians counts as
none when it is no larger than the span of the --reps calls of one parent process; every call's figure is kept.

    python tools/sort_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile] [--parent-lib PATH --parent-commit ID]
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
from lookup_probe import L, NLINES, WIDTH, key_columns, fill_set, timed, upload

PATTERN = rb"k=([a-z]+) v=([0-9]+)"
KEY_GROUP, SORT_GROUP = [1], 2
DIGITS = 18
HEAD = b"GET /index.html k="
# passes: (values a buffer spreads over, size of the route by key's set with as many passes or None)
RANGES = {1: (256, 200), 3: (1 << 24, 200000), 4: (1 << 32, None), 8: (10 ** 18, None)}
LIMITS = (0, 100)


def fill_lines(lib, span, size):
    """the buffer: line i = HEAD, the key i % size, " v=", its number in 18 digits, a tail of x, a newline; returns
    (buffer, bytes, the numbers)"""
    row = np.frombuffer((HEAD + b"a" * WIDTH + b" v=" + b"0" * DIGITS + b" user nobody " + b"x" * L)[:L - 1] + b"\n", dtype=np.uint8)
    a = np.tile(row, (NLINES, 1))
    i = np.arange(NLINES, dtype=np.uint64)
    for j, col in enumerate(key_columns((i % np.uint64(size)).astype(np.int64))):
        a[:, len(HEAD) + j] = col
    v = ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(3)) % np.uint64(span)
    v[0], v[1] = 0, span - 1            # the range is exactly the one that takes the passes
    at, rest = len(HEAD) + WIDTH + 3, v.copy()
    for j in range(DIGITS - 1, -1, -1):
        a[:, at + j] = (rest % np.uint64(10)).astype(np.uint8) + ord("0")
        rest //= np.uint64(10)
    buf, nbytes = upload(lib, a.tobytes())
    return buf, nbytes, v.astype(np.int64)


def sort_call(sc, buf, nbytes, out, desc, limit, index=None):
    return sc.sort_lines(buf.ptr, nbytes, out.ptr, nbytes, SORT_GROUP, descending=desc, limit=limit,
                         index_ptr=index.ptr if index else None, index_cap=NLINES if index else 0)


def host_tail(sc, buf, nbytes, out, perm, lib, desc):
    """(c): the field on the device, its rows to the host, a stable argsort there, the permutation back"""
    info = sc.extract_lines(buf.ptr, nbytes, [SORT_GROUP], out.ptr, nbytes)
    rows = np.frombuffer(out.to_bytes(info.out_bytes), dtype=np.uint8).reshape(-1, DIGITS + 1)
    v = (rows[:, :DIGITS].astype(np.int64) - ord("0")) @ (10 ** np.arange(DIGITS - 1, -1, -1, dtype=np.int64))
    order = np.argsort(-v if desc else v, kind="stable")
    raw = np.ascontiguousarray(order.astype(np.int64)).tobytes()
    step = 32 << 20
    for o in range(0, len(raw), step):
        assert lib.sre_hip_upload(perm.ptr + o, raw[o:o + step], len(raw[o:o + step])) == 0
    return order


def run_range(lib, pool, prog, passes, reps):
    span, size = RANGES[passes]
    buf, nbytes, v = fill_lines(lib, span, size or 200)
    assert nbytes == NLINES * L
    out, index, keyid, buckets = (S.DeviceBuffer(nbytes), S.DeviceBuffer(48 * NLINES), S.DeviceBuffer(8 * NLINES),
                                  S.DeviceBuffer(40 * NLINES))
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    ks = None
    if size:
        dbuf, dbytes = fill_set(lib, size)
        ks = S.KeySet(dbuf.ptr, dbytes, 1)
    configs = [(desc, limit) for desc in (False, True) for limit in LIMITS]
    t = {c: [] for c in configs}
    t.update({"filter": [], "route_key": [], "host": []})
    orders = {}
    for rep in range(reps + 1):             # (the first round warms up: code objects, buffers)
        sc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes)
        for desc, limit in (configs if rep % 2 == 0 else configs[::-1]):
            d, info = timed(lambda: sort_call(sc, buf, nbytes, out, desc, limit))
            nout = limit or NLINES
            assert sc.last_lines_device == 1 and info == S.SortInfo(NLINES, NLINES, NLINES, nout, nout * L, nout, nout * L, passes,
                                                                    0, span - 1), info
            if rep == 0 and limit == 0:
                assert sort_call(sc, buf, nbytes, out, desc, limit, index) == info
                orders[desc] = np.frombuffer(index.to_bytes(48 * NLINES), dtype=np.int64).reshape(-1, 6)[:, 0].copy()
            elif rep:
                t[(desc, limit)].append(d)
        d, finfo = timed(lambda: sc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes))
        assert finfo.nwritten == NLINES
        if rep:
            t["filter"].append(d)
        if ks:
            d, rinfo = timed(lambda: sc.route_lines_by_key(buf.ptr, nbytes, out.ptr, nbytes, KEY_GROUP, ks, keyid_ptr=keyid.ptr,
                                                           keyid_cap=NLINES, buckets_ptr=buckets.ptr, buckets_cap=NLINES))
            assert rinfo.nwritten == NLINES and rinfo.nbuckets == size
            if rep:
                t["route_key"].append(d)
        d, order = timed(lambda: host_tail(sc, buf, nbytes, out, index, lib, rep % 2 == 1))
        if rep < 2:
            # the device's order is the host's stable sort, line by line, in both directions
            assert (orders[rep % 2 == 1] == order).all()
            assert (v[order[:-1]] <= v[order[1:]]).all() if rep % 2 == 0 else (v[order[:-1]] >= v[order[1:]]).all()
        if rep:
            t["host"].append(d)
    med = statistics.median
    host_span = (max(t["host"]) - min(t["host"])) * 1e3
    row = {"passes": passes, "values": span, "lines": NLINES, "bytes": nbytes, "kernel": sc.kernel_name,
           "sort_ms": {("desc" if desc else "asc") + "_limit_%d" % limit: ms(t[(desc, limit)]) for desc, limit in configs},
           "filter_lines_ms": ms(t["filter"]),
           "route_lines_by_key_ms": ms(t["route_key"]) if ks else None, "route_by_key_set_keys": size,
           "host_extract_download_argsort_upload_ms": ms(t["host"]), "host_tail_span_ms": host_span}
    s = med(t[(False, 0)])
    row["sort_minus_filter_ms"] = (s - med(t["filter"])) * 1e3
    row["sort_over_host_tail"] = s / med(t["host"])
    row["sort_below_host_tail_by_more_than_its_span"] = all((med(t["host"]) - med(t[c])) * 1e3 > host_span for c in configs)
    if ks:
        row["sort_minus_route_by_key_ms"] = (s - med(t["route_key"])) * 1e3
        ks.close()
        dbuf.free()
    for b in (buf, out, index, keyid, buckets):
        b.free()
    return row


def child(calls):
    """the run to put under the profiler: per range `calls` sort calls and route by key calls after one warm-up call each"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        out, keyid, buckets = S.DeviceBuffer(NLINES * L), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(40 * NLINES)
        for passes, (span, size) in RANGES.items():
            buf, nbytes, _ = fill_lines(lib, span, size or 200)
            for _ in range(calls + 1):
                sort_call(sc, buf, nbytes, out, False, 0)
            if size:
                dbuf, dbytes = fill_set(lib, size)
                ks = S.KeySet(dbuf.ptr, dbytes, 1)
                for _ in range(calls + 1):
                    sc.route_lines_by_key(buf.ptr, nbytes, out.ptr, nbytes, KEY_GROUP, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES,
                                          buckets_ptr=buckets.ptr, buckets_cap=NLINES)
                ks.close()
                dbuf.free()
            buf.free()


def short_name(name):
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    return name.split("(")[0]


def profile(calls, stats_out):
    """the child under rocprofv3: per range and call the kernels of a call, microseconds and dispatches per call"""
    tmp = tempfile.mkdtemp(prefix="sort_probe_")
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
        # kernel of either sink and is dropped)
        per_call, cur = [], None
        for r in rows:
            name = short_name(r["Kernel_Name"])
            if name.endswith("sre_k_lines_count"):
                cur = {}
                per_call.append(cur)
            if cur is not None:
                us, n = cur.get(name, (0, 0))
                cur[name] = (us + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), n + 1)
        per_call = [c for c in per_call if any("k_sort_" in n or "route_key" in n for n in c)]
        configs = [(passes, call) for passes, (_, size) in RANGES.items() for call in (("sort", "route_by_key") if size else ("sort",))]
        assert len(per_call) == len(configs) * (calls + 1), (len(per_call), calls)
        out = []
        for i, (passes, call) in enumerate(configs):
            mine = per_call[i * (calls + 1) + 1:(i + 1) * (calls + 1)]
            names = sorted({n for c in mine for n in c})
            kernels = {n: {"us": statistics.median([c.get(n, (0, 0))[0] for c in mine]) / 1e3, "dispatches": mine[0].get(n, (0, 0))[1]}
                       for n in names}
            part = sum(v["us"] for n, v in kernels.items() if "partition_count" in n or "partition_scatter" in n)
            out.append({"passes": passes, "call": call, "kernels": kernels, "count_and_scatter_us": part,
                        "count_and_scatter_us_per_pass": part / passes,
                        "all_kernels_us": statistics.median([sum(v[0] for v in c.values()) for c in mine]) / 1e3})
        with open(stats[0], newline="") as f:
            top = stats_top(csv.DictReader(f), 24)
        return out, top
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def older(reps):
    """lookup_lines, route_lines_by_key, tally_sums_lines and sort_lines with whatever library this process loaded"""
    lib = S.load_library()
    size = 4096
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        dbuf, dbytes = fill_set(lib, size)
        ks = S.KeySet(dbuf.ptr, dbytes, 1)
        buf, nbytes, _ = fill_lines(lib, 1 << 24, size)
        out, keyid, buckets = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(40 * NLINES)
        sums = S.DeviceBuffer(32 * size)
        tl, tr, tt, ts = [], [], [], []
        for rep in range(reps + 1):
            d, info = timed(lambda: sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, KEY_GROUP, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES))
            assert info.nwritten == NLINES
            tl.append(d)
            d, rinfo = timed(lambda: sc.route_lines_by_key(buf.ptr, nbytes, out.ptr, nbytes, KEY_GROUP, ks, keyid_ptr=keyid.ptr,
                                                           keyid_cap=NLINES, buckets_ptr=buckets.ptr, buckets_cap=NLINES))
            assert rinfo.nwritten == NLINES and rinfo.nbuckets == size
            tr.append(d)
            d, tinfo = timed(lambda: sc.tally_sums_lines(buf.ptr, nbytes, out.ptr, nbytes, KEY_GROUP, [SORT_GROUP], NLINES,
                                                         sums_ptr=sums.ptr, sums_cap=size))
            assert tinfo.nkeys == size
            tt.append(d)
            d, sinfo = timed(lambda: sort_call(sc, buf, nbytes, out, False, 0))
            assert sinfo.nwritten == NLINES and sinfo.passes == 3
            ts.append(d)
        print(json.dumps({"lookup_ms": ms(tl[1:]), "route_lines_by_key_ms": ms(tr[1:]), "tally_sums_ms": ms(tt[1:]),
                          "sort_lines_ms": ms(ts[1:])}))


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
    for metric in ("lookup_ms", "route_lines_by_key_ms", "tally_sums_ms", "sort_lines_ms"):
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
    doc = {"tool": "tools/sort_probe.py", "parent_commit": args.parent_commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps after a warm-up; sort_lines (the lines, no index) in "
                     "both directions with limit 0 and 100, filter_lines on the same buffer, route_lines_by_key by the key group "
                     "with a set that takes as many passes (1 and 3) and extract_lines of the number + download + a stable numpy "
                     "argsort + upload of the permutation alternating in one process; every line carries an 18-digit number",
           "pattern": PATTERN.decode(), "sort_group": SORT_GROUP, "results": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        for passes in RANGES:
            r = run_range(lib, pool, prog, passes, args.reps)
            print(json.dumps(r), flush=True)
            doc["results"].append(r)
    by = {r["passes"]: r["sort_ms"]["asc_limit_0"]["median"] for r in doc["results"]}
    doc["ms_per_added_pass"] = {"from": "(8 passes - 1 pass) / 7, whole calls ascending with limit 0; the kernels' own times are under "
                                        "`kernels`", "value": (by[8] - by[1]) / 7}
    if not args.no_profile:
        per, top = profile(3, args.stats_out)
        doc["kernels"] = {"run": "sort_lines ascending with limit 0, and route_lines_by_key where a set takes as many passes, under "
                                 "rocprofv3 --kernel-trace --stats, in a run of its own: 3 calls each per range after a warm-up call, "
                                 "whose dispatches are left out; median microseconds per call and kernel, and the dispatches of a call",
                          "kernel_stats_top": top, "rows": per}
    if args.parent_lib:
        doc["older_calls_parent_vs_branch"] = {
            "run": "lookup_lines, route_lines_by_key (4096 keys each), tally_sums_lines (4096 keys, one value column) and sort_lines "
                   "(ascending, no limit, 2^24 values: three passes) over a million lines in child processes that load the parent commit's library and this tree's in turn (parent, branch, "
                   "parent, branch); medians of reps after a warm-up",
            "rows": older_ab(args.parent_lib, args.reps)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
