"""The line filter against line mode on the same buffer (sre_hip_filter_lines vs sre_hip_scan_lines).

A million 96-byte lines (the lines of lines_probe.py) with 0 %, 25 % and 100 % of the lines selected, Thompson and
FIRST, on the table-driven scanner and on the NFA tier.  Per configuration
  (a) the whole filter_lines call (no index) and
  (b) scan_lines with cap = nlines
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after
a warm-up.  Then (c): one run of the table-driven FIRST scanner at 25 % and 100 % under rocprofv3 --kernel-trace
--stats in a child process; its kernel statistics go to --stats-out, and the gather kernel's time per dispatch
gives its rate, (selected bytes read + bytes written) / kernel time, next to sre_hip_read_ceiling on the same box
in the same run.  Prints one JSON document (--out also writes it to a file).

    python tools/filter_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile]
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
from lines_probe import LINES, NFA_LINES, NFA_PATTERN, PATTERN, fill_repeat, read_ceiling, time_lines

NLINES = 1 << 20
PERCENTS = (0, 25, 100)
ENGINES = {"scan": (PATTERN, LINES, S.ENGINE_AUTO, S.ENGINE_SCAN), "nfa": (NFA_PATTERN, NFA_LINES, S.ENGINE_NFA, S.ENGINE_NFA)}
MODES = ((S.HIP_THOMPSON, "thompson"), (S.HIP_PIKE_FIRST, "first"))
GATHER = "sre_k_lines_gather"


def block_of(lines, percent):
    """four lines, `percent` of them with a match"""
    return {0: lines["nomatch"] * 4, 25: lines["match"] + lines["nomatch"] * 3, 100: lines["match"] * 4}[percent]


def time_filter(sc, buf, nbytes, out, cap):
    info = (ctypes.c_size_t * 5)()
    t0 = time.perf_counter()
    assert sc.lib.sre_hip_filter_lines(sc.h, buf.ptr, nbytes, 0x0A, 0, out.ptr, cap, None, 0, info, None) == 0
    return time.perf_counter() - t0, S.FilterInfo(*info)


def ms(xs):
    return {"median": statistics.median(xs) * 1e3, "min": min(xs) * 1e3, "all": [x * 1e3 for x in xs]}


def run_config(lib, pool, prog, engine, routed, lines, mode, percent, reps):
    block = block_of(lines, percent)
    nbytes = len(block) // 4 * NLINES
    buf = fill_repeat(lib, nbytes, block)
    out = S.DeviceBuffer(nbytes)
    sc = S.Scanner(pool, prog, mode, engine)
    assert sc.engine == routed
    rows = (ctypes.c_ssize_t * (NLINES * (3 + sc.slots)))()
    ta, tb = [], []
    for rep in range(reps + 1):         # (the first round warms up: code objects, buffers)
        da, info = time_filter(sc, buf, nbytes, out, nbytes)
        fdev, fkms = sc.last_lines_device, sc.last_kernel_ms
        db, nl, nr = time_lines(sc, buf, nbytes, NLINES, rows)
        assert nl == info.nlines == NLINES and nr == info.nselected == info.nwritten == NLINES * percent // 100, (nl, nr, info)
        assert info.out_bytes == info.need_bytes == nr * (len(block) // 4)
        assert fdev == sc.last_lines_device == 1
        if rep:
            ta.append(da)
            tb.append(db)
    row = {"percent_selected": percent, "selected": nr, "bytes": nbytes, "out_bytes": info.out_bytes, "kernel": sc.kernel_name,
           "filter_ms": ms(ta), "scan_lines_ms": ms(tb), "scan_kernels_ms": fkms,
           "filter_over_scan_lines": statistics.median(ta) / statistics.median(tb)}
    buf.free()
    out.free()
    return row


def child(percents, calls):
    """the run to put under the profiler: the table-driven FIRST scanner, `calls` filter calls per selectivity after
    one warm-up call each"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        for percent in percents:
            block = block_of(LINES, percent)
            nbytes = len(block) // 4 * NLINES
            buf = fill_repeat(lib, nbytes, block)
            out = S.DeviceBuffer(nbytes)
            for _ in range(calls + 1):
                time_filter(sc, buf, nbytes, out, nbytes)
            buf.free()
            out.free()


def profile(percents, calls, stats_out):
    """(c): the child under rocprofv3; the gather's dispatches in order, `calls + 1` per selectivity"""
    tmp = tempfile.mkdtemp(prefix="filter_probe_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", ",".join(str(p) for p in percents), "--child-calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert stats and trace, os.listdir(tmp)
        if stats_out:
            shutil.copyfile(stats[0], stats_out)
        with open(trace[0], newline="") as f:
            rows = [r for r in csv.DictReader(f) if GATHER in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
        assert len(ns) == len(percents) * (calls + 1), (len(ns), percents, calls)
        with open(stats[0], newline="") as f:
            top = [{"name": r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0], "calls": int(r["Calls"]),
                    "total_ns": int(r["TotalDurationNs"]), "percent": float(r["Percentage"])} for r in csv.DictReader(f)][:12]
        return {p: ns[i * (calls + 1) + 1:(i + 1) * (calls + 1)] for i, p in enumerate(percents)}, top
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-out", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-calls", type=int, default=5, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        child([int(p) for p in args.child.split(",")], args.child_calls)
        return
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    doc = {"tool": "tools/filter_probe.py", "commit": commit, "reps": args.reps, "lines": NLINES, "line_bytes": 96,
           "timing": "host clock around each synchronous call; median of reps after a warm-up, filter_lines and scan_lines "
                     "(cap = nlines) alternating in one process",
           "patterns": {"scan": PATTERN.decode(), "nfa": NFA_PATTERN.decode()}, "results": {}}
    nbytes = 96 * NLINES
    buf = fill_repeat(lib, nbytes, LINES["match"])
    doc["read_ceiling_GBps"] = read_ceiling(lib, buf, nbytes, reps=5)
    buf.free()
    with S.Pool() as pool:
        for ename, (pattern, lines, engine, routed) in ENGINES.items():
            prog = S.compile(pool, S.parse(pool, [pattern]))
            for mode, mname in MODES:
                rows = [run_config(lib, pool, prog, engine, routed, lines, mode, p, args.reps) for p in PERCENTS]
                # the yardstick: scan_lines with a match on every line, in the same run
                yard = rows[-1]["scan_lines_ms"]["median"]
                for r in rows:
                    r["filter_over_scan_lines_at_100"] = r["filter_ms"]["median"] / yard
                    print(json.dumps({ename: {mname: r}}), flush=True)
                doc["results"].setdefault(ename, {})[mname] = rows
    if not args.no_profile:
        per, top = profile([25, 100], 5, args.stats_out)
        doc["gather_kernel"] = {"run": "table-driven FIRST scanner under rocprofv3 --kernel-trace --stats, 5 calls per selectivity "
                                       "after a warm-up call", "kernel_stats_top": top, "rows": []}
        for p, ns in per.items():
            moved = 2 * 96 * (NLINES * p // 100)        # selected bytes read + bytes written (len + 1 each way)
            med = statistics.median(ns)
            doc["gather_kernel"]["rows"].append({"percent_selected": p, "bytes_read_plus_written": moved, "kernel_us": [x / 1e3 for x in ns],
                                                 "median_us": med / 1e3, "GBps": moved / med,
                                                 "fraction_of_read_ceiling": moved / med / doc["read_ceiling_GBps"]})
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
