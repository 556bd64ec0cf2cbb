"""The line substitute against line mode on the same buffer (sre_hip_substitute_lines vs sre_hip_scan_lines).

A million 96-byte log lines with 0 %, 25 % and 100 % of them holding a URI, the URI program in mode FIRST on the
table-driven scanner, template $1://$2/*** (the path and the query masked).  Per selectivity
  (a) the whole substitute_lines call with all_lines (sed 's/../../': every line comes back, no index),
  (b) scan_lines with cap = nlines, which is how a caller gets the match and its captures without this call (the
      rewrite on the host and the upload of the text are not even counted), and
  (c) filter_lines with all_lines: the same lines moved with no piece table,
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after
a warm-up.  Then one run at 25 % and 100 % under rocprofv3 --kernel-trace --stats in a child process that calls
substitute_lines and filter_lines on the same lines; its kernel statistics go to --stats-out, and the two gather
kernels' times per dispatch give their rates, (bytes read + bytes written) / kernel time, next to
sre_hip_read_ceiling on the same box in the same run.  Prints one JSON document (--out also writes it to a file).

    python tools/subst_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile]
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
from extract_probe import LINES, NLINES, PATTERN, PERCENTS, L, block_of, stats_top
from filter_probe import ms
from lines_probe import fill_repeat, read_ceiling, time_lines

TEMPLATE = b"$1://$2/***"
ROWS = {"nomatch": LINES["nomatch"], "match": LINES["match"].replace(b"http://abc.cc/ab/c?a=b", b"http://abc.cc/***")}
GATHERS = {"substitute": "sre_k_subst_gather", "filter": "sre_k_lines_gather"}
ALL = S.HIP_LINES_ALL


def expected_block(percent):
    return {0: ROWS["nomatch"] * 4, 25: ROWS["match"] + ROWS["nomatch"] * 3, 100: ROWS["match"] * 4}[percent]


def time_subst(sc, buf, nbytes, out, cap):
    info = (ctypes.c_size_t * 5)()
    t0 = time.perf_counter()
    assert sc.lib.sre_hip_substitute_lines(sc.h, buf.ptr, nbytes, 0x0A, TEMPLATE, len(TEMPLATE), ALL, out.ptr, cap, None, 0, info,
                                           None) == 0
    return time.perf_counter() - t0, S.FilterInfo(*info)


def time_filter_all(sc, buf, nbytes, out, cap):
    info = (ctypes.c_size_t * 5)()
    t0 = time.perf_counter()
    assert sc.lib.sre_hip_filter_lines(sc.h, buf.ptr, nbytes, 0x0A, ALL, out.ptr, cap, None, 0, info, None) == 0
    return time.perf_counter() - t0, S.FilterInfo(*info)


def run_config(lib, pool, prog, percent, reps):
    block = block_of(percent)
    nbytes = L * NLINES
    buf = fill_repeat(lib, nbytes, block)
    out = S.DeviceBuffer(nbytes)
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    rows = (ctypes.c_ssize_t * (NLINES * (3 + sc.slots)))()
    want = expected_block(percent)
    ta, tb, tc = [], [], []
    for rep in range(reps + 1):         # (the first round warms up: code objects, buffers)
        da, info = time_subst(sc, buf, nbytes, out, nbytes)
        dev, kms = sc.last_lines_device, sc.last_kernel_ms
        if rep == 0:
            head = ctypes.create_string_buffer(len(want))
            assert lib.sre_hip_download(head, out.ptr, len(want)) == 0
            assert head.raw == want, head.raw
        db, nl, nr = time_lines(sc, buf, nbytes, NLINES, rows)
        dc, finfo = time_filter_all(sc, buf, nbytes, out, nbytes)
        assert nl == info.nlines == NLINES and nr == NLINES * percent // 100, (nl, nr, info)
        assert info.nselected == info.nwritten == finfo.nwritten == NLINES
        assert info.out_bytes == info.need_bytes == len(want) * NLINES // 4 and finfo.out_bytes == nbytes
        assert dev == sc.last_lines_device == 1
        if rep:
            ta.append(da)
            tb.append(db)
            tc.append(dc)
    row = {"percent_matched": percent, "matched": nr, "bytes": nbytes, "out_bytes": info.out_bytes, "kernel": sc.kernel_name,
           "substitute_ms": ms(ta), "scan_lines_ms": ms(tb), "filter_all_ms": ms(tc), "scan_kernels_ms": kms,
           "rows_bytes_scan_lines_copies_to_the_host": nr * (3 + sc.slots) * 8,
           "substitute_over_scan_lines": statistics.median(ta) / statistics.median(tb),
           "substitute_over_filter_all": statistics.median(ta) / statistics.median(tc)}
    buf.free()
    out.free()
    return row


def child(percents, calls):
    """the run to put under the profiler: `calls` substitute and filter calls per selectivity after one warm-up call each"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        for percent in percents:
            nbytes = L * NLINES
            buf = fill_repeat(lib, nbytes, block_of(percent))
            out = S.DeviceBuffer(nbytes)
            for _ in range(calls + 1):
                time_subst(sc, buf, nbytes, out, nbytes)
                time_filter_all(sc, buf, nbytes, out, nbytes)
            buf.free()
            out.free()


def profile(percents, calls, stats_out):
    """the child under rocprofv3; each gather's dispatches in order, `calls + 1` per selectivity"""
    tmp = tempfile.mkdtemp(prefix="subst_probe_")
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
    doc = {"tool": "tools/subst_probe.py", "commit": commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps after a warm-up; substitute_lines (all lines), "
                     "scan_lines (cap = nlines) and filter_lines (all lines) alternating in one process",
           "pattern": PATTERN.decode(), "template": TEMPLATE.decode(), "row": ROWS["match"].decode(), "results": []}
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
        doc["gather_kernels"] = {"run": "substitute_lines and filter_lines (all lines) alternating on the same lines under rocprofv3 "
                                        "--kernel-trace --stats, 5 calls of each per selectivity after a warm-up call",
                                 "kernel_stats_top": top, "rows": []}
        for which in GATHERS:
            for p, ns in per[which].items():
                written = len(expected_block(p)) * NLINES // 4 if which == "substitute" else nbytes
                # the substitute reads what it writes, less the literal bytes of the matched lines; the filter moves whole lines
                moved = 2 * written - (NLINES * p // 100) * 7 if which == "substitute" else 2 * nbytes
                med = statistics.median(ns)
                doc["gather_kernels"]["rows"].append({"gather": which, "kernel": GATHERS[which], "percent_matched": p,
                                                      "bytes_written": written, "bytes_read_plus_written": moved,
                                                      "kernel_us": [x / 1e3 for x in ns], "median_us": med / 1e3, "GBps": moved / med,
                                                      "written_GBps": written / med,
                                                      "fraction_of_read_ceiling": moved / med / doc["read_ceiling_GBps"]})
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
