"""The line sort by text against the calls a user has without it (sre_hip_sort_lines_text vs sre_hip_filter_lines,
sre_hip_sort_lines and extract + download + a numpy sort + upload).

A million 96-byte log lines `GET k=KEY v=NUMBER xxx..`, the program k=([^ ]+) v=([0-9]+) in mode FIRST on the table-driven
scanner, sort group 1.  Four workloads:
  key7      keys of 7 letters: one chunk, 7 passes;
  dotted    dotted addresses of 7 to 15 bytes: three chunks;
  path40    paths of 40 bytes: six chunks, 40 passes;
  path40_8  the same keys with max_bytes = 8: two chunks, 8 passes.
No key holds a NUL (numpy's S type ignores trailing NULs).  Per workload
  (s) the whole sort_lines_text call (the lines; no index), ascending and descending, with limit 0 and limit 100,
  (a) filter_lines on the same buffer, which writes the same lines in line order: the same bytes moved, no sort,
  (b) where the plan has at most 8 passes, sort_lines on the numeric group, whose numbers are spread over a range that takes as
      many passes,
  (c) the host alternative: extract_lines of the key, a download of the rows, a stable argsort of the byte strings in numpy (an
      S-dtype array: unsigned bytes) and an upload of the permutation.  The library has no call that gathers lines by a
      permutation, so the gather the user would still need is NOT in (c): (c) is a lower bound of the alternative
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after a
warm-up.  A round begins with one untimed filter_lines call, because the first device call behind the host work of (c) is slow
whichever call it is.  Then, in a run of its own, the child under rocprofv3 --kernel-trace --stats makes (s) ascending with
limit 0 on every workload.

--parent-lib PATH: the condition that the calls whose digit driver changed cost what they cost before.  sort_lines (a 1-pass
and an 8-pass range), tally_top_lines (4096 keys, by count) and route_lines_by_key (4096 keys, the control: its passes are its
own) are timed in child processes that load PATH (a build of the parent commit, through SREGEX_AMD_LIB) and this tree's library
in turn: parent, branch, parent, branch.  A difference between the medians counts as none when it is no larger than the span
of the --reps calls of one parent process; every call's figure is kept.

    python tools/sort_text_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile] [--parent-lib PATH --parent-commit ID]
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
from lookup_probe import L, NLINES, fill_set, timed, upload
import sort_probe
import tally_top_probe

PATTERN = rb"k=([^ ]+) v=([0-9]+)"
TEXT_GROUP, NUMBER_GROUP = 1, 2
DIGITS = 18
LIMITS = (0, 100)
# name: (key length or None for the dotted addresses, max_bytes, passes of the plan)
WORKLOADS = {"key7": (7, 0, 7), "dotted": (None, 0, None), "path40": (40, 0, 40), "path40_8": (40, 8, 8)}


def letters(i, width, salt):
    """NLINES x width lowercase letters, spread by a multiplicative hash; about NLINES / 4 distinct keys"""
    h = ((i % np.uint64(NLINES // 4)) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    cols = np.empty((len(i), width), dtype=np.uint8)
    for j in range(width):
        cols[:, j] = ((h >> np.uint64((j * 5) % 59)) % np.uint64(26)).astype(np.uint8) + ord("a")
    return cols


def fill_lines(lib, name):
    """the buffer of a workload; returns (buffer, bytes, the keys as an S array, the numbers' span)"""
    width, max_bytes, passes = WORKLOADS[name]
    i = np.arange(NLINES, dtype=np.uint64)
    span = 1 << 24 if passes is None or passes > 8 else min(1 << (8 * passes), 10 ** 18) if passes < 8 else 10 ** 18
    v = ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(3)) % np.uint64(span)
    v[0], v[1] = 0, span - 1
    if width is None:
        h = (i % np.uint64(NLINES // 4)) * np.uint64(0x9E3779B97F4A7C15)
        octets = [((h >> np.uint64(11 * k + 7)) % np.uint64(256)).astype(np.int64) for k in range(4)]
        octets[3][::64] %= 10           # (and some short ones)
        octets[2][::64] %= 10
        octets[1][::64] %= 10
        octets[0][::64] %= 10
        keys = np.array([b"%d.%d.%d.%d" % o for o in zip(*octets)], dtype="S15")
        lines = [b"GET k=" + k + b" v=%018d " % int(n) for k, n in zip(keys.tolist(), v.tolist())]
        raw = b"".join(t + b"x" * (L - 1 - len(t)) + b"\n" for t in lines)
    else:
        cols = letters(i, width, 17)
        cols[:, 0] = ord("/") if width == 40 else cols[:, 0]
        head, mid = b"GET k=", b" v="
        row = np.frombuffer((head + b"a" * width + mid + b"0" * DIGITS + b" " + b"x" * L)[:L - 1] + b"\n", dtype=np.uint8)
        a = np.tile(row, (NLINES, 1))
        a[:, len(head):len(head) + width] = cols
        at, rest = len(head) + width + len(mid), v.copy()
        for j in range(DIGITS - 1, -1, -1):
            a[:, at + j] = (rest % np.uint64(10)).astype(np.uint8) + ord("0")
            rest //= np.uint64(10)
        raw = a.tobytes()
        keys = np.ascontiguousarray(cols).view("S%d" % width).reshape(-1)
    assert len(raw) == NLINES * L
    buf, nbytes = upload(lib, raw)
    return buf, nbytes, keys, span


def stable_order(keys, desc):
    """numpy's stable argsort of the byte strings; descending keeps equal keys in line order too"""
    if not desc:
        return np.argsort(keys, kind="stable")
    return (len(keys) - 1 - np.argsort(keys[::-1], kind="stable"))[::-1]


def text_call(sc, buf, nbytes, out, max_bytes, desc, limit, index=None):
    return sc.sort_lines_text(buf.ptr, nbytes, out.ptr, nbytes, TEXT_GROUP, max_bytes=max_bytes, descending=desc, limit=limit,
                              index_ptr=index.ptr if index else None, index_cap=NLINES if index else 0)


def host_tail(sc, buf, nbytes, out, perm, lib, width, max_bytes, desc):
    """(c): the key on the device, its rows to the host, a stable argsort of the byte strings there, the permutation back"""
    info = sc.extract_lines(buf.ptr, nbytes, [TEXT_GROUP], out.ptr, nbytes)
    raw = out.to_bytes(info.out_bytes)
    if width is None:
        keys = np.array(raw.split(b"\n")[:-1], dtype="S15")
    else:
        rows = np.frombuffer(raw, dtype=np.uint8).reshape(-1, width + 1)
        take = max_bytes or width
        keys = np.ascontiguousarray(rows[:, :take]).view("S%d" % take).reshape(-1)
    order = stable_order(keys, desc)
    data = np.ascontiguousarray(order.astype(np.int64)).tobytes()
    step = 32 << 20
    for o in range(0, len(data), step):
        assert lib.sre_hip_upload(perm.ptr + o, data[o:o + step], len(data[o:o + step])) == 0
    return order


def run_workload(lib, pool, prog, name, reps):
    width, max_bytes, _ = WORKLOADS[name]
    buf, nbytes, keys, span = fill_lines(lib, name)
    cut = keys.astype("S%d" % max_bytes) if max_bytes else keys
    lens = np.char.str_len(cut)
    plan = S.sort_text_plan(int(lens.min()), int(lens.max()), False)
    out, index = S.DeviceBuffer(nbytes), S.DeviceBuffer(48 * NLINES)
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    numeric = len(plan) <= 8
    configs = [(desc, limit) for desc in (False, True) for limit in LIMITS]
    t = {c: [] for c in configs}
    t.update({"filter": [], "numeric": [], "host": []})
    orders = {}
    for rep in range(reps + 1):             # (the first round warms up: code objects, buffers)
        sc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes)
        for desc, limit in (configs if rep % 2 == 0 else configs[::-1]):
            d, info = timed(lambda: text_call(sc, buf, nbytes, out, max_bytes, desc, limit))
            nout = limit or NLINES
            assert sc.last_lines_device == 1 and info == S.SortTextInfo(NLINES, NLINES, nout, nout * L, nout, nout * L, len(plan),
                                                                        int(lens.min()), int(lens.max())), info
            if rep == 0 and limit == 0:
                assert text_call(sc, buf, nbytes, out, max_bytes, desc, limit, index) == info
                orders[desc] = np.frombuffer(index.to_bytes(48 * NLINES), dtype=np.int64).reshape(-1, 6)[:, 0].copy()
            elif rep:
                t[(desc, limit)].append(d)
        d, finfo = timed(lambda: sc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes))
        assert finfo.nwritten == NLINES
        if rep:
            t["filter"].append(d)
        if numeric:
            d, ninfo = timed(lambda: sc.sort_lines(buf.ptr, nbytes, out.ptr, nbytes, NUMBER_GROUP))
            assert ninfo.nwritten == NLINES and ninfo.passes == len(plan), ninfo
            if rep:
                t["numeric"].append(d)
        d, order = timed(lambda: host_tail(sc, buf, nbytes, out, index, lib, width, max_bytes, rep % 2 == 1))
        if rep < 2:
            # the device's order is the host's stable sort, line by line, in both directions
            assert (orders[rep % 2 == 1] == order).all()
        if rep:
            t["host"].append(d)
    med = statistics.median
    host_span = (max(t["host"]) - min(t["host"])) * 1e3
    row = {"workload": name, "key_bytes": [int(lens.min()), int(lens.max())], "max_bytes": max_bytes, "passes": len(plan),
           "chunks": len({c for c, _ in plan}), "lines": NLINES, "bytes": nbytes, "kernel": sc.kernel_name,
           "sort_text_ms": {("desc" if desc else "asc") + "_limit_%d" % limit: ms(t[(desc, limit)]) for desc, limit in configs},
           "filter_lines_ms": ms(t["filter"]), "sort_lines_same_passes_ms": ms(t["numeric"]) if numeric else None,
           "host_extract_download_argsort_upload_ms": ms(t["host"]), "host_span_ms": host_span}
    s = med(t[(False, 0)])
    row["sort_text_minus_filter_ms"] = (s - med(t["filter"])) * 1e3
    row["ms_per_pass_over_filter"] = (s - med(t["filter"])) * 1e3 / len(plan)
    row["sort_text_over_host"] = s / med(t["host"])
    row["sort_text_below_host_by_more_than_its_span"] = all((med(t["host"]) - med(t[c])) * 1e3 > host_span for c in configs)
    if numeric:
        row["sort_text_minus_sort_lines_ms"] = (s - med(t["numeric"])) * 1e3
    for b in (buf, out, index):
        b.free()
    return row


def child(calls):
    """the run to put under the profiler: per workload `calls` calls after a warm-up call"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        out = S.DeviceBuffer(NLINES * L)
        for name, (_, max_bytes, _) in WORKLOADS.items():
            buf, nbytes, _, _ = fill_lines(lib, name)
            for _ in range(calls + 1):
                text_call(sc, buf, nbytes, out, max_bytes, False, 0)
            buf.free()


def profile(calls, stats_out):
    """the child under rocprofv3: per workload the kernels of a call, microseconds and dispatches per call"""
    tmp = tempfile.mkdtemp(prefix="sort_text_probe_")
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
        # a call of the scanner begins with the split's first kernel
        per_call, cur = [], None
        for r in rows:
            name = sort_probe.short_name(r["Kernel_Name"])
            if name.endswith("sre_k_lines_count"):
                cur = {}
                per_call.append(cur)
            if cur is not None:
                us, n = cur.get(name, (0, 0))
                cur[name] = (us + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), n + 1)
        per_call = [c for c in per_call if any("k_sort_text" in n for n in c)]
        assert len(per_call) == len(WORKLOADS) * (calls + 1), (len(per_call), calls)
        out = []
        for i, name in enumerate(WORKLOADS):
            mine = per_call[i * (calls + 1) + 1:(i + 1) * (calls + 1)]
            names = sorted({n for c in mine for n in c})
            kernels = {n: {"us": statistics.median([c.get(n, (0, 0))[0] for c in mine]) / 1e3, "dispatches": mine[0].get(n, (0, 0))[1]}
                       for n in names}
            part = sum(v["us"] for n, v in kernels.items() if "partition_count" in n or "partition_scatter" in n)
            npass = max(sum(v["dispatches"] for n, v in kernels.items() if "partition_count" in n), 1)
            out.append({"workload": name, "kernels": kernels, "count_and_scatter_us": part, "digit_passes": npass,
                        "count_and_scatter_us_per_pass": part / npass,
                        "keys_us": sum(v["us"] for n, v in kernels.items() if "k_sort_text_keys" in n),
                        "all_kernels_us": statistics.median([sum(v[0] for v in c.values()) for c in mine]) / 1e3})
        with open(stats[0], newline="") as f:
            top = stats_top(csv.DictReader(f), 24)
        return out, top
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


OLDER = ("sort_lines_1_pass_ms", "sort_lines_8_passes_ms", "tally_top_lines_4096_keys_ms", "route_lines_by_key_ms")


def older(reps):
    """sort_lines (1 and 8 passes), tally_top_lines and route_lines_by_key with whatever library this process loaded"""
    lib = S.load_library()
    size = 4096
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [sort_probe.PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        dbuf, dbytes = fill_set(lib, size)
        ks = S.KeySet(dbuf.ptr, dbytes, 1)
        one, nbytes, _ = sort_probe.fill_lines(lib, 256, size)
        eight, _, _ = sort_probe.fill_lines(lib, 10 ** 18, size)
        out, keyid, buckets = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(40 * NLINES)
        counts, sums = S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(32 * NLINES)
        t = {m: [] for m in OLDER}
        for rep in range(reps + 1):
            d, info = timed(lambda: sort_probe.sort_call(sc, one, nbytes, out, False, 0))
            assert info.nwritten == NLINES and info.passes == 1
            t[OLDER[0]].append(d)
            d, info = timed(lambda: sort_probe.sort_call(sc, eight, nbytes, out, False, 0))
            assert info.nwritten == NLINES and info.passes == 8
            t[OLDER[1]].append(d)
            d, info = timed(lambda: tally_top_probe.top_call(sc, one, nbytes, out, counts, sums, S.HIP_TOP_COUNT, 0))
            assert info.nkeys == size
            t[OLDER[2]].append(d)
            d, info = timed(lambda: sc.route_lines_by_key(one.ptr, nbytes, out.ptr, nbytes, [1], ks, keyid_ptr=keyid.ptr,
                                                          keyid_cap=NLINES, buckets_ptr=buckets.ptr, buckets_cap=NLINES))
            assert info.nwritten == NLINES and info.nbuckets == size
            t[OLDER[3]].append(d)
        print(json.dumps({m: ms(v[1:]) for m, v in t.items()}))


def older_ab(parent_lib, reps):
    """parent, branch, parent, branch in child processes of their own; per call the runs and whether the difference of the
    medians lies inside the span of one parent process's calls"""
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
    for metric in OLDER:
        p_runs = [r[metric]["all"] for w, r in runs if w == "parent"]
        p = [r[metric]["median"] for w, r in runs if w == "parent"]
        b = [r[metric]["median"] for w, r in runs if w == "branch"]
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
    doc = {"tool": "tools/sort_text_probe.py", "parent_commit": args.parent_commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps after a warm-up; sort_lines_text (the lines, no index) "
                     "in both directions with limit 0 and 100, filter_lines on the same buffer, sort_lines on the numeric group over a "
                     "range that takes as many passes (plans of at most 8) and extract_lines of the key + download + a stable numpy "
                     "argsort of the byte strings + upload of the permutation alternating in one process.  The host alternative has "
                     "no gather of the lines: the library has no call for it, so its figure is a lower bound",
           "pattern": PATTERN.decode(), "sort_group": TEXT_GROUP, "results": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        for name in WORKLOADS:
            r = run_workload(lib, pool, prog, name, args.reps)
            print(json.dumps(r), flush=True)
            doc["results"].append(r)
    by = {r["workload"]: r for r in doc["results"]}
    a, b = by["key7"], by["path40"]
    doc["ms_per_added_pass"] = {"from": "(path40 - key7) / (their passes' difference), whole calls ascending with limit 0, which includes "
                                        "the keys of five more chunks; the kernels' own times are under `kernels`",
                                "value": (b["sort_text_ms"]["asc_limit_0"]["median"] - a["sort_text_ms"]["asc_limit_0"]["median"])
                                / (b["passes"] - a["passes"])}
    if not args.no_profile:
        per, top = profile(3, args.stats_out)
        doc["kernels"] = {"run": "sort_lines_text ascending with limit 0 under rocprofv3 --kernel-trace --stats, in a run of its own: 3 "
                                 "calls per workload after a warm-up call, whose dispatches are left out; median microseconds per call "
                                 "and kernel, and the dispatches of a call",
                          "kernel_stats_top": top, "rows": per}
    if args.parent_lib:
        doc["older_calls_parent_vs_branch"] = {
            "run": "sort_lines (ascending, no limit; 256 values: one pass, 10^18 values: eight), tally_top_lines (4096 keys, by count, "
                   "descending) and route_lines_by_key (4096 keys; the control) over a million lines in child processes that load the "
                   "parent commit's library and this tree's in turn (parent, branch, parent, branch); medians of reps after a warm-up",
            "rows": older_ab(args.parent_lib, args.reps)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
