"""The line filter with context lines against the line filter on the same buffer (sre_hip_filter_lines_context vs
sre_hip_filter_lines).

A million 96-byte lines (the lines of lines_probe.py), 1 % and 25 % of them with a match, the table-driven FIRST
scanner.  Per (before, after) in (0, 0), (2, 2), (0, 100), (100000, 100000) three calls alternate in one process, each
timed by the host clock around the synchronous call, the median of --reps rounds after a warm-up round:
  (a) filter_lines_context(before, after), no index;
  (b) filter_lines on the same matches (what the call costs without the context pass and with the matched lines only);
  (c) filter_lines with the flags (none, invert or all_lines) whose output is closest in bytes to (a)'s: the same
      scan and a gather that moves a comparable number of bytes.
The selected lines are checked against a numpy dilation.  Prints one JSON document (--out also writes it to a file).

    python tools/context_probe.py [--reps 5] [--out FILE] [--commit TEXT]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sregex_amd as S
from lines_probe import LINES, PATTERN, fill_repeat

NLINES = 1 << 20
L = 96
CONTEXTS = ((0, 0), (2, 2), (0, 100), (100000, 100000))
PERIODS = {1: 100, 25: 4}           # percent of lines with a match: one line in so many


def dilate(matched, before, after):
    idx = np.arange(len(matched), dtype=np.int64)
    big = np.int64(1) << 62
    p = np.maximum.accumulate(np.where(matched, idx, -big))
    q = np.minimum.accumulate(np.where(matched, idx, big)[::-1])[::-1]
    return (idx - p <= after) | (q - idx <= before)


def time_context(sc, buf, nbytes, out, before, after):
    info = (ctypes.c_size_t * 7)()
    t0 = time.perf_counter()
    assert sc.lib.sre_hip_filter_lines_context(sc.h, buf.ptr, nbytes, 0x0A, 0, before, after, out.ptr, nbytes, None, 0, info, None) == 0
    return time.perf_counter() - t0, S.ContextInfo(*info)


def time_filter(sc, buf, nbytes, out, flags):
    info = (ctypes.c_size_t * 5)()
    t0 = time.perf_counter()
    assert sc.lib.sre_hip_filter_lines(sc.h, buf.ptr, nbytes, 0x0A, flags, out.ptr, nbytes, None, 0, info, None) == 0
    return time.perf_counter() - t0, S.FilterInfo(*info)


def ms(xs):
    return {"median": statistics.median(xs) * 1e3, "min": min(xs) * 1e3, "all": [x * 1e3 for x in xs]}


def run_config(lib, sc, percent, reps):
    period = PERIODS[percent]
    block = LINES["match"] + LINES["nomatch"] * (period - 1)
    nbytes = L * NLINES
    buf = fill_repeat(lib, nbytes, block)
    out = S.DeviceBuffer(nbytes)
    matched = np.arange(NLINES) % period == 0
    nmatched = int(matched.sum())
    flag_sets = {"none": (0, nmatched), "invert": (S.HIP_LINES_INVERT, NLINES - nmatched), "all_lines": (S.HIP_LINES_ALL, NLINES)}
    rows = []
    for before, after in CONTEXTS:
        sel = dilate(matched, before, after)
        nsel = int(sel.sum())
        ngroups = int((sel & ~np.concatenate(([False], sel[:-1]))).sum())
        comparable = min(flag_sets, key=lambda k: abs(flag_sets[k][1] - nsel))
        ta, tb, tc = [], [], []
        for rep in range(reps + 1):         # (the first round warms up: code objects, buffers)
            da, info = time_context(sc, buf, nbytes, out, before, after)
            assert sc.last_lines_device == 1
            db, same = time_filter(sc, buf, nbytes, out, 0)
            dc, comp = time_filter(sc, buf, nbytes, out, flag_sets[comparable][0])
            assert info == S.ContextInfo(NLINES, nmatched, nsel, ngroups, nsel * L, nsel, nsel * L), (info, nsel, ngroups)
            assert same == S.FilterInfo(NLINES, nmatched, nmatched * L, nmatched, nmatched * L), same
            assert comp.nselected == flag_sets[comparable][1] and comp.out_bytes == comp.nselected * L
            if rep:
                ta.append(da)
                tb.append(db)
                tc.append(dc)
        row = {"percent_matched": percent, "before": before, "after": after, "matched": nmatched, "selected": nsel, "groups": ngroups,
               "out_bytes": nsel * L, "context_ms": ms(ta), "filter_same_matches_ms": ms(tb), "filter_same_matches_out_bytes": nmatched * L,
               "filter_comparable_flags": comparable, "filter_comparable_out_bytes": comp.out_bytes, "filter_comparable_ms": ms(tc),
               "context_over_filter_same_matches": statistics.median(ta) / statistics.median(tb),
               "context_over_filter_comparable": statistics.median(ta) / statistics.median(tc)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    buf.free()
    out.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git rev-parse HEAD)")
    args = ap.parse_args()
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = None
    doc = {"tool": "tools/context_probe.py", "commit": commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps rounds after a warm-up round; filter_lines_context, "
                     "filter_lines on the same matches and filter_lines with the flags that move a comparable number of bytes "
                     "alternate in one process",
           "pattern": PATTERN.decode(), "scanner": "table-driven, HIP_PIKE_FIRST", "results": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        assert sc.engine == S.ENGINE_SCAN
        for percent in PERIODS:
            doc["results"] += run_config(lib, sc, percent, args.reps)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
