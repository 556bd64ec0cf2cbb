"""The line route against what a caller can do without it (sre_hip_route_lines vs sre_hip_filter_lines / sre_hip_scan_lines).

A million 96-byte lines, four rules plus rest on the table-driven scanner, at three rule mixes: one rule takes every
line, each rule takes a quarter, 1 % of the lines are routed (a quarter of them to each rule) and the rest dropped.
Per mix
  (r) the whole route_lines call (no index),
  (a) filter_lines with the same four-rule scanner, which writes the same number of lines: it moves the same bytes and
      is the floor,
  (b) what a caller does today: four filter_lines calls with single-rule scanners, one output after the other,
  (c) scan_lines with cap = nlines (the rows a caller would regroup on the host)
alternate in one process, each timed by the host clock around the synchronous call(s): the median of --reps rounds
after a warm-up round.  Then one run of the route at the three mixes under rocprofv3 --kernel-trace --stats in a child
process; its kernel statistics go to --stats-out.  Prints one JSON document (--out also writes it to a file).

    python tools/route_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile]
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sregex_amd as S
from lines_probe import fill_repeat, time_lines

NLINES = 1 << 20
L = 96
WORDS = [b"alpha", b"bravo", b"charlie", b"delta"]
RULES = [w + b"@[a-z]+" for w in WORDS]
MIXES = ("one", "quarter", "1pct")


def line(word):
    return (b"GET /index.html user " + word + b" " + b"x" * L)[:L - 1] + b"\n"


def block_of(mix):
    rule = [line(w + b"@abc") for w in WORDS]
    rest = line(b"nobody")
    if mix == "one":
        return rule[0]
    if mix == "quarter":
        return b"".join(rule)
    return b"".join(rule[k] + rest * 99 for k in range(4))          # 1 % routed


def bucket_map(mix):
    return [0, 1, 2, 3, -1] if mix == "1pct" else [0, 1, 2, 3, 4]


def time_route(sc, buf, nbytes, out, cap, m, nb):
    arr = (ctypes.c_int * len(m))(*m)
    info = (ctypes.c_size_t * 5)()
    bk = (ctypes.c_size_t * (3 * nb))()
    t0 = time.perf_counter()
    assert sc.lib.sre_hip_route_lines(sc.h, buf.ptr, nbytes, 0x0A, arr, nb, out.ptr, cap, None, 0, info, bk, None) == 0
    return time.perf_counter() - t0, S.FilterInfo(*info), [bk[3 * b] for b in range(nb)]


def time_filter(sc, buf, nbytes, out_ptr, cap):
    info = (ctypes.c_size_t * 5)()
    t0 = time.perf_counter()
    assert sc.lib.sre_hip_filter_lines(sc.h, buf.ptr, nbytes, 0x0A, 0, out_ptr, cap, None, 0, info, None) == 0
    return time.perf_counter() - t0, S.FilterInfo(*info)


def ms(xs):
    return {"median": statistics.median(xs) * 1e3, "min": min(xs) * 1e3, "all": [x * 1e3 for x in xs]}


def scanners(pool):
    prog = S.compile(pool, S.parse(pool, RULES, multi=True))
    multi = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert multi.engine == S.ENGINE_SCAN
    singles = [S.Scanner(pool, S.compile(pool, S.parse(pool, [r])), S.HIP_PIKE_FIRST) for r in RULES]
    return multi, singles


def run_mix(lib, multi, singles, mix, reps):
    block = block_of(mix)
    nbytes = L * NLINES
    buf = fill_repeat(lib, nbytes, block)
    out = S.DeviceBuffer(nbytes)
    m = bucket_map(mix)
    rows = (ctypes.c_ssize_t * (NLINES * (3 + multi.slots)))()
    tr, ta, tb, tc = [], [], [], []
    for rep in range(reps + 1):         # (the first round warms up: code objects, buffers)
        dr, info, per = time_route(multi, buf, nbytes, out, nbytes, m, 5)
        assert multi.last_lines_device == 1
        da, finfo = time_filter(multi, buf, nbytes, out.ptr, nbytes)
        assert finfo.nselected == info.nselected == info.nwritten and finfo.need_bytes == info.need_bytes == info.out_bytes
        db, at = 0.0, 0
        for k, sc in enumerate(singles):
            d, sinfo = time_filter(sc, buf, nbytes, out.ptr + at, nbytes - at)
            assert sinfo.nselected == sinfo.nwritten == per[k], (k, sinfo, per)
            db += d
            at += sinfo.out_bytes
        dc, nl, nr = time_lines(multi, buf, nbytes, NLINES, rows)
        assert nl == NLINES and nr == finfo.nselected
        if rep:
            tr.append(dr)
            ta.append(da)
            tb.append(db)
            tc.append(dc)
    med = statistics.median
    row = {"mix": mix, "bytes": nbytes, "routed": info.nselected, "out_bytes": info.out_bytes, "bucket_lines": per,
           "route_ms": ms(tr), "filter_same_lines_ms": ms(ta), "four_filters_ms": ms(tb), "scan_lines_ms": ms(tc),
           "route_over_filter": med(tr) / med(ta), "route_over_four_filters": med(tr) / med(tb),
           "route_over_scan_lines": med(tr) / med(tc), "route_minus_filter_ms": (med(tr) - med(ta)) * 1e3}
    buf.free()
    out.free()
    return row


def child(calls):
    """the run to put under the profiler: `calls` route calls per mix after one warm-up call each"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, RULES, multi=True))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        nbytes = L * NLINES
        out = S.DeviceBuffer(nbytes)
        for mix in MIXES:
            buf = fill_repeat(lib, nbytes, block_of(mix))
            for _ in range(calls + 1):
                time_route(sc, buf, nbytes, out, nbytes, bucket_map(mix), 5)
            buf.free()
        out.free()


def profile(calls, stats_out):
    """the child under rocprofv3; per kernel of the route its dispatches in order, `calls + 1` per mix"""
    tmp = tempfile.mkdtemp(prefix="route_probe_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--child-calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert stats and trace, os.listdir(tmp)
        if stats_out:
            shutil.copyfile(stats[0], stats_out)
        with open(trace[0], newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        # a call begins with the split's first kernel; the calls of a mix are consecutive
        per_call, cur = [], None
        for r in rows:
            name = r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
            if name.endswith("sre_k_lines_count"):
                cur = {}
                per_call.append(cur)
            if cur is not None:
                cur[name] = cur.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        assert len(per_call) == len(MIXES) * (calls + 1), (len(per_call), calls)
        out = {}
        for i, mix in enumerate(MIXES):
            mine = per_call[i * (calls + 1) + 1:(i + 1) * (calls + 1)]
            names = sorted({n for c in mine for n in c})
            out[mix] = {n: statistics.median([c.get(n, 0) for c in mine]) / 1e3 for n in names}
            out[mix]["all_kernels"] = statistics.median([sum(c.values()) for c in mine]) / 1e3
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-out", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-calls", type=int, default=5, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child_calls)
        return
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    doc = {"tool": "tools/route_probe.py", "commit": commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "rules": [r.decode() for r in RULES], "buckets": 5,
           "timing": "host clock around each synchronous call; median of reps after a warm-up round; route_lines, filter_lines "
                     "(same scanner), four single-rule filter_lines calls and scan_lines (cap = nlines) alternating in one process",
           "results": []}
    with S.Pool() as pool:
        multi, singles = scanners(pool)
        for mix in MIXES:
            row = run_mix(lib, multi, singles, mix, args.reps)
            print(json.dumps(row), flush=True)
            doc["results"].append(row)
    if not args.no_profile:
        doc["route_kernels_us"] = {"run": "the route alone under rocprofv3 --kernel-trace --stats, 5 calls per mix after a warm-up "
                                          "call; median microseconds per call and kernel", "mixes": profile(5, args.stats_out)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
