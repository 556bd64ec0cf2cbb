#!/usr/bin/env python3
"""bench.py with two or more builds of the library in alternating child processes on one box: the parent commit's
against this tree's, or one source built with different switches.  Boxes differ by several percent on the same binary, so
a difference counts only inside one call of this tool, and only when it is outside the spread of the runs of one build.

usage: ab_bench.py --lib parent=PATH/libsregex.so --lib branch= [--lib NAME=PATH ...] [--runs 4] [--timeout 300]
                   [--out FILE] [-- bench.py arguments]
An empty PATH is this tree's own library (no SREGEX_AMD_LIB).  The builds take turns in the order given, --runs times.
Every child runs under its own time limit; the tool stops at the first child that does not exit with status 0 (what
was measured up to there is still written) and returns that status.  "separated" says whether EVERY run of a build lies
below every run of the first one.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    argv = sys.argv[1:]
    bench_args = []
    if "--" in argv:
        bench_args = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True, metavar="NAME=PATH")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    libs = [tuple(s.split("=", 1)) for s in args.lib]
    for name, path in libs:
        if path and not os.path.exists(path):
            raise SystemExit("%s: no such library: %s" % (name, path))
    runs = {name: [] for name, _ in libs}
    status = 0
    for turn in range(args.runs):
        for name, path in libs:
            env = dict(os.environ)
            env.pop("SREGEX_AMD_LIB", None)
            if path:
                env["SREGEX_AMD_LIB"] = os.path.abspath(path)
            t0 = time.time()
            try:
                p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bench_args, env=env, cwd=ROOT,
                                   stdout=subprocess.PIPE, timeout=args.timeout)
                status = p.returncode
            except subprocess.TimeoutExpired:
                status = 124
            if status != 0:
                print("%s run %d: status %d, stopping" % (name, turn, status), file=sys.stderr)
                break
            line = json.loads(p.stdout.decode().strip().splitlines()[-1])
            runs[name].append({"ms_per_step": line["ms_per_step"], "kernel_ms": line["roofline"].get("kernel_ms"),
                               "kernel": line["roofline"].get("kernel"), "GBps": line["value"],
                               "matches": line["config"]["matches"], "fixup_rounds": line["config"]["fixup_rounds"]})
            print("%-8s run %d: %.4f ms per step, kernel %s ms (%.0f s)"
                  % (name, turn, line["ms_per_step"], line["roofline"].get("kernel_ms"), time.time() - t0), flush=True)
        if status != 0:
            break
    base = libs[0][0]
    out = {"bench_args": bench_args, "order": [n for n, _ in libs], "status": status, "runs": runs, "summary": {}}
    for name, _ in libs:
        ms = [r["ms_per_step"] for r in runs[name]]
        if not ms:
            continue
        s = {"median_ms_per_step": statistics.median(ms), "min": min(ms), "max": max(ms)}
        km = [r["kernel_ms"] for r in runs[name] if r["kernel_ms"] is not None]
        if km:
            s["median_kernel_ms"] = statistics.median(km)
        if name != base and runs[base]:
            b = [r["ms_per_step"] for r in runs[base]]
            s["median_ratio_to_" + base] = statistics.median(ms) / statistics.median(b)
            s["separated"] = max(ms) < min(b)
            s["slower_beyond_spread"] = min(ms) > max(b)
        out["summary"][name] = s
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out["summary"]))
    return status


if __name__ == "__main__":
    sys.exit(main())
