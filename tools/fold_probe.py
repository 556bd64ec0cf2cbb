"""The line fold against the line filter on the same buffer (sre_hip_fold_lines vs sre_hip_filter_lines with SRE_HIP_LINES_ALL).

A million 96-byte lines (the lines of lines_probe.py), the table-driven FIRST scanner, three shapes of records: every line
its own record (nothing marked), records of 2 .. 8 lines, and one record of a million lines; both modes (a marked line
belongs to the previous line / continues into the next).  Per configuration
  (a) the whole fold_lines call (no tables, and with both tables),
  (b) filter_lines with SRE_HIP_LINES_ALL, which moves the same bytes: the yardstick,
  (c) the host alternative: filter_lines with an index of every marked line, the index downloaded, the fold in numpy on the
      host, the separator bytes uploaded (one byte per line; the text itself stays on the device, so this is a floor)
alternate in one process, each timed by the host clock around the synchronous calls: the median of --reps rounds after a
warm-up.  Then one run of the 2 .. 8 shape under rocprofv3 --kernel-trace --stats in a child process; its kernel statistics go
to --stats-out.  With --parent-lib PATH, filter_lines, filter_lines_context and extract_lines are timed in child processes
that load PATH (a build of the parent commit, through SREGEX_AMD_LIB) and this tree's library in turn: parent, branch,
parent, branch.  Prints one JSON document (--out also writes it to a file).

    python tools/fold_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile] [--parent-lib PATH --parent-commit ID]
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sregex_amd as S
from lines_probe import LINES, PATTERN, read_ceiling

NLINES = 1 << 20
L = 96
SHAPES = ("single", "two_to_eight", "one_record")


def shape_text(shape, nxt):
    """NLINES lines of L bytes; a line with a match is MARKED.  Returns (text, records)"""
    rng = random.Random(5)
    m, u = LINES["match"], LINES["nomatch"]
    if shape == "single":
        return u * NLINES, NLINES
    if shape == "one_record":
        return (m * (NLINES - 1) + u) if nxt else (u + m * (NLINES - 1)), 1
    parts, n, recs = [], 0, 0
    while n < NLINES:
        k = min(rng.randrange(2, 9), NLINES - n)
        parts.append(m * (k - 1) + u if nxt else u + m * (k - 1))
        n += k
        recs += 1
    return b"".join(parts), recs


def upload(lib, text):
    buf = S.DeviceBuffer(len(text))
    step = 32 << 20
    for o in range(0, len(text), step):
        piece = text[o:o + step]
        assert lib.sre_hip_upload(buf.ptr + o, piece, len(piece)) == 0
    return buf


def ms(xs):
    return {"median": statistics.median(xs) * 1e3, "min": min(xs) * 1e3, "all": [x * 1e3 for x in xs]}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def host_fold(sc, lib, buf, nbytes, out, idx, h_idx, sep, nxt):
    """the host alternative: which lines are marked comes down as index rows, the fold is numpy's, one separator byte per
    line goes up"""
    info = sc.filter_lines(buf.ptr, nbytes, None, 0, index_ptr=None, index_cap=0)       # sizing: how many rows
    rows = info.nselected
    if rows:
        # (the index needs an output to describe: the marked lines are written too, as the only call there was would)
        info = sc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes, index_ptr=idx.ptr, index_cap=rows)
        assert lib.sre_hip_download(h_idx.ctypes.data_as(ctypes.c_void_p), idx.ptr, 32 * rows) == 0
    marked = np.zeros(NLINES, dtype=bool)
    marked[h_idx[:4 * rows:4]] = True
    head = np.ones(NLINES, dtype=bool)
    if nxt:
        head[1:] = ~marked[:-1]
    else:
        head[1:] = ~marked[1:]
    last = np.ones(NLINES, dtype=bool)
    last[:-1] = head[1:]
    seps = np.where(last, np.uint8(0x0A), np.uint8(0x01))
    assert lib.sre_hip_upload(sep.ptr, seps.ctypes.data_as(ctypes.c_void_p), NLINES) == 0
    return int(head.sum())


def run_config(lib, pool, prog, shape, nxt, reps):
    text, recs = shape_text(shape, nxt)
    nbytes = len(text)
    assert nbytes == L * NLINES
    buf = upload(lib, text)
    out = S.DeviceBuffer(nbytes + 16)
    rid, rec = S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(40 * NLINES)
    idx, sep = S.DeviceBuffer(32 * NLINES), S.DeviceBuffer(NLINES)
    h_idx = np.zeros(4 * NLINES, dtype=np.int64)
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    t = {"fold": [], "fold_tables": [], "filter_all": [], "host": []}
    for rep in range(reps + 1):         # (the first round warms up: code objects, buffers)
        d, info = timed(lambda: sc.fold_lines(buf.ptr, nbytes, out.ptr, out.nbytes, fold_next=nxt))
        assert (info.nlines, info.nrecords, info.nwritten, info.out_bytes) == (NLINES, recs, recs, nbytes), info
        assert sc.last_lines_device == 1
        kms = sc.last_kernel_ms
        d2, info2 = timed(lambda: sc.fold_lines(buf.ptr, nbytes, out.ptr, out.nbytes, fold_next=nxt, recid_ptr=rid.ptr, recid_cap=NLINES,
                                                records_ptr=rec.ptr, records_cap=NLINES))
        assert info2 == info
        d3, f = timed(lambda: sc.filter_lines(buf.ptr, nbytes, out.ptr, out.nbytes, all_lines=True))
        assert f.nselected == NLINES and f.out_bytes == nbytes
        d4, hrecs = timed(lambda: host_fold(sc, lib, buf, nbytes, out, idx, h_idx, sep, nxt))
        assert hrecs == recs
        if rep:
            for k, v in zip(("fold", "fold_tables", "filter_all", "host"), (d, d2, d3, d4)):
                t[k].append(v)
    row = {"shape": shape, "mode": "next" if nxt else "previous", "records": recs, "longest": info.longest, "marked": info.nmarked,
           "bytes": nbytes, "scan_kernels_ms": kms, "fold_ms": ms(t["fold"]), "fold_with_tables_ms": ms(t["fold_tables"]),
           "filter_all_ms": ms(t["filter_all"]), "host_alternative_ms": ms(t["host"]),
           "fold_minus_filter_all_us": (statistics.median(t["fold"]) - statistics.median(t["filter_all"])) * 1e6,
           "host_over_fold": statistics.median(t["host"]) / statistics.median(t["fold"])}
    for b in (buf, out, rid, rec, idx, sep):
        b.free()
    return row


def child(calls):
    """the run to put under the profiler: records of 2 .. 8 lines, `calls` fold calls with both tables after a warm-up"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        text, _ = shape_text("two_to_eight", False)
        buf = upload(lib, text)
        out, rid, rec = S.DeviceBuffer(len(text) + 16), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(40 * NLINES)
        for _ in range(calls + 1):
            sc.fold_lines(buf.ptr, len(text), out.ptr, out.nbytes, recid_ptr=rid.ptr, recid_cap=NLINES, records_ptr=rec.ptr,
                          records_cap=NLINES)
            sc.filter_lines_context(buf.ptr, len(text), out.ptr, out.nbytes, 1, 1)


def profile(calls, stats_out):
    tmp = tempfile.mkdtemp(prefix="fold_probe_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--child-calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        assert stats, os.listdir(tmp)
        if stats_out:
            shutil.copyfile(stats[0], stats_out)
        with open(stats[0], newline="") as f:
            return [{"name": r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0], "calls": int(r["Calls"]),
                     "total_ns": int(r["TotalDurationNs"]), "average_ns": float(r.get("AverageNs") or 0), "percent": float(r["Percentage"])}
                    for r in csv.DictReader(f)][:24]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def older(reps):
    """the calls that existed before, in this process's library: one JSON line"""
    lib = S.load_library()
    text, _ = shape_text("two_to_eight", False)
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        buf, out = upload(lib, text), S.DeviceBuffer(len(text) + 16)
        calls = {"filter_lines": lambda: sc.filter_lines(buf.ptr, len(text), out.ptr, out.nbytes),
                 "filter_lines_context": lambda: sc.filter_lines_context(buf.ptr, len(text), out.ptr, out.nbytes, 1, 2),
                 "extract_lines": lambda: sc.extract_lines(buf.ptr, len(text), [1, 2], out.ptr, out.nbytes)}
        t = {k: [] for k in calls}
        for rep in range(reps + 1):
            for k, fn in calls.items():
                d, _ = timed(fn)
                if rep:
                    t[k].append(d)
        print(json.dumps({k: ms(v) for k, v in t.items()}))


def older_ab(parent_lib, reps):
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
    for metric in runs[0][1]:
        p_runs = [r[metric]["all"] for w, r in runs if w == "parent"]
        p = [r[metric]["median"] for w, r in runs if w == "parent"]
        b = [r[metric]["median"] for w, r in runs if w == "branch"]
        spread = max(max(x) for x in p_runs) - min(min(x) for x in p_runs)
        diff = statistics.mean(b) - statistics.mean(p)
        rows.append({"metric": metric, "parent_medians_ms": p, "branch_medians_ms": b, "parent_runs_ms": p_runs,
                     "branch_minus_parent_ms": diff, "parent_spread_ms": spread, "difference_within_parent_spread": abs(diff) <= spread})
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
    ap.add_argument("--child-calls", type=int, default=5, help=argparse.SUPPRESS)
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
    doc = {"tool": "tools/fold_probe.py", "parent_commit": args.parent_commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps rounds after a warm-up round; fold_lines, fold_lines with "
                     "both tables, filter_lines with SRE_HIP_LINES_ALL and the host alternative alternating in one process",
           "pattern": PATTERN.decode(), "rows": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        probe = upload(lib, LINES["match"] * NLINES)
        doc["read_ceiling_GBps"] = read_ceiling(lib, probe, L * NLINES, reps=5)
        probe.free()
        for shape in SHAPES:
            for nxt in (False, True):
                row = run_config(lib, pool, prog, shape, nxt, args.reps)
                print(json.dumps(row), flush=True)
                doc["rows"].append(row)
    if not args.no_profile:
        doc["kernels"] = {"run": "records of 2 .. 8 lines under rocprofv3 --kernel-trace --stats: 6 fold_lines calls with both tables and 6 "
                                 "filter_lines_context calls (before = after = 1) on the same buffer", "kernel_stats_top": profile(5, args.stats_out)}
    if args.parent_lib:
        doc["older_calls_parent_vs_branch"] = {
            "run": "filter_lines, filter_lines_context and extract_lines on the 2 .. 8 buffer in child processes that load the parent "
                   "commit's library and this tree's in turn (parent, branch, parent, branch); medians of reps after a warm-up",
            "rows": older_ab(args.parent_lib, args.reps)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
