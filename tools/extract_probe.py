"""The line extract against line mode on the same buffer (sre_hip_extract_lines vs sre_hip_scan_lines).

A million 96-byte log lines with 0 %, 25 % and 100 % of them holding a URI, the URI program in mode FIRST on the
table-driven scanner, groups [1, 2, 3, 4] (scheme, host, path, query).  Per selectivity
  (a) the whole extract_lines call (no index) and
  (b) scan_lines with cap = nlines, which is how a caller gets the captures without this call,
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after
a warm-up.  Then (c): one run at 25 % and 100 % under rocprofv3 --kernel-trace --stats in a child process that calls
extract_lines and filter_lines on the same lines; its kernel statistics go to --stats-out, and the two gather
kernels' times per dispatch give their rates, (source bytes read + bytes written) / kernel time, next to
sre_hip_read_ceiling on the same box in the same run.  Prints one JSON document (--out also writes it to a file).

    python tools/extract_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile]
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
from filter_probe import ms, time_filter
from lines_probe import fill_repeat, read_ceiling, time_lines

NLINES = 1 << 20
L = 96
PERCENTS = (0, 25, 100)
PATTERN = rb"([a-z]+)://([^/ ]+)(/[^ ?]*)?(\?[^ ]*)?"
GROUPS = [1, 2, 3, 4]
LINES = {"nomatch": (b"GET /index.html user nobody " + b"x" * L)[:L - 1] + b"\n",
         "match": (b"GET http://abc.cc/ab/c?a=b user nobody " + b"x" * L)[:L - 1] + b"\n"}
ROW = b"http\tabc.cc\t/ab/c\t?a=b\n"
GATHERS = {"extract": "sre_k_extract_gather", "filter": "sre_k_lines_gather"}


def block_of(percent):
    """four lines, `percent` of them with a URI"""
    return {0: LINES["nomatch"] * 4, 25: LINES["match"] + LINES["nomatch"] * 3, 100: LINES["match"] * 4}[percent]


def time_extract(sc, buf, nbytes, out, cap):
    info = (ctypes.c_size_t * 5)()
    groups = (ctypes.c_int * len(GROUPS))(*GROUPS)
    t0 = time.perf_counter()
    assert sc.lib.sre_hip_extract_lines(sc.h, buf.ptr, nbytes, 0x0A, groups, len(GROUPS), 0x09, 0, out.ptr, cap, None, 0, info,
                                        None) == 0
    return time.perf_counter() - t0, S.FilterInfo(*info)


def run_config(lib, pool, prog, percent, reps):
    block = block_of(percent)
    nbytes = L * NLINES
    buf = fill_repeat(lib, nbytes, block)
    out = S.DeviceBuffer(nbytes)
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    rows = (ctypes.c_ssize_t * (NLINES * (3 + sc.slots)))()
    ta, tb = [], []
    for rep in range(reps + 1):         # (the first round warms up: code objects, buffers)
        da, info = time_extract(sc, buf, nbytes, out, nbytes)
        dev, kms = sc.last_lines_device, sc.last_kernel_ms
        db, nl, nr = time_lines(sc, buf, nbytes, NLINES, rows)
        assert nl == info.nlines == NLINES and nr == info.nselected == info.nwritten == NLINES * percent // 100, (nl, nr, info)
        assert info.out_bytes == info.need_bytes == nr * len(ROW)
        assert dev == sc.last_lines_device == 1
        if rep:
            ta.append(da)
            tb.append(db)
    if nr:
        head = ctypes.create_string_buffer(2 * len(ROW))
        assert lib.sre_hip_download(head, out.ptr, 2 * len(ROW)) == 0
        assert head.raw == ROW * 2, head.raw
    row = {"percent_selected": percent, "selected": nr, "bytes": nbytes, "out_bytes": info.out_bytes, "kernel": sc.kernel_name,
           "extract_ms": ms(ta), "scan_lines_ms": ms(tb), "scan_kernels_ms": kms,
           "rows_bytes_scan_lines_copies_to_the_host": nr * (3 + sc.slots) * 8,
           "extract_over_scan_lines": statistics.median(ta) / statistics.median(tb)}
    buf.free()
    out.free()
    return row


def child(percents, calls):
    """the run to put under the profiler: `calls` extract and filter calls per selectivity after one warm-up call each"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        for percent in percents:
            nbytes = L * NLINES
            buf = fill_repeat(lib, nbytes, block_of(percent))
            out = S.DeviceBuffer(nbytes)
            for _ in range(calls + 1):
                time_extract(sc, buf, nbytes, out, nbytes)
                time_filter(sc, buf, nbytes, out, nbytes)
            buf.free()
            out.free()


def stats_top(rows, n=14):
    """the first n rows of a rocprofv3 kernel_stats.csv, the kernel names without namespace and arguments"""
    return [{"name": r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0], "calls": int(r["Calls"]),
             "total_ns": int(r["TotalDurationNs"]), "percent": float(r["Percentage"])} for r in rows][:n]


def profile(percents, calls, stats_out):
    """(c): the child under rocprofv3; each gather's dispatches in order, `calls + 1` per selectivity"""
    tmp = tempfile.mkdtemp(prefix="extract_probe_")
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
            all_rows = list(csv.DictReader(f))
        per = {}
        for which, name in GATHERS.items():
            rows = sorted((r for r in all_rows if name in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
            ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
            assert len(ns) == len(percents) * (calls + 1), (which, len(ns), percents, calls)
            per[which] = {p: ns[i * (calls + 1) + 1:(i + 1) * (calls + 1)] for i, p in enumerate(percents)}
        with open(stats[0], newline="") as f:
            top = stats_top(csv.DictReader(f))
        return per, top
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
    doc = {"tool": "tools/extract_probe.py", "commit": commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps after a warm-up, extract_lines and scan_lines "
                     "(cap = nlines) alternating in one process",
           "pattern": PATTERN.decode(), "groups": GROUPS, "row": ROW.decode(), "results": []}
    nbytes = L * NLINES
    buf = fill_repeat(lib, nbytes, LINES["match"])
    doc["read_ceiling_GBps"] = read_ceiling(lib, buf, nbytes, reps=5)
    buf.free()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        for p in PERCENTS:
            r = run_config(lib, pool, prog, p, args.reps)
            print(json.dumps(r), flush=True)
            doc["results"].append(r)
    if not args.no_profile:
        per, top = profile([25, 100], 5, args.stats_out)
        doc["gather_kernels"] = {"run": "extract_lines and filter_lines alternating on the same lines under rocprofv3 --kernel-trace "
                                        "--stats, 5 calls of each per selectivity after a warm-up call",
                                 "kernel_stats_top": top, "rows": []}
        for which in GATHERS:
            for p, ns in per[which].items():
                sel = NLINES * p // 100
                # the extract reads the fields' bytes and writes them with a separator each; the filter moves whole lines
                moved = sel * ((len(ROW) - len(GROUPS)) + len(ROW)) if which == "extract" else 2 * L * sel
                med = statistics.median(ns)
                doc["gather_kernels"]["rows"].append({"gather": which, "kernel": GATHERS[which], "percent_selected": p,
                                                      "bytes_written": sel * (len(ROW) if which == "extract" else L),
                                                      "bytes_read_plus_written": moved, "kernel_us": [x / 1e3 for x in ns],
                                                      "median_us": med / 1e3, "GBps": moved / med,
                                                      "written_GBps": sel * (len(ROW) if which == "extract" else L) / med,
                                                      "fraction_of_read_ceiling": moved / med / doc["read_ceiling_GBps"]})
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
