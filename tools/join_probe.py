"""The line join against the calls a user has without it (sre_hip_join_lines vs sre_hip_lookup_lines and lookup + download +
a Python join).

A million 96-byte log lines, each with k=KEY (five letters), the program k=([a-z]+) in mode FIRST on the table-driven
scanner, group [1] (the lines of tools/lookup_probe.py).  A key map holds the keys 0 .. S - 1 for S = 1, 4096 and 2^20 with
V = 1 or 4 value columns of 8 bytes each; every line is a member (line i: key i % S).  Per map size and V
  (a) the whole join_lines call (rows and key ids; no index),
  (b) lookup_lines on the same map, which selects the same lines (lines and key ids; no index), and
  (e) the host alternative: lookup_lines with index rows, a download of the index and the key ids, and a Python join over
      the host's copy of the lines
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after a
warm-up.  Then, in a run of its own, (c) and (d): the child under rocprofv3 --kernel-trace --stats makes calls (a) and (b);
the join pass is listed next to the lookup's probe pass, and the join's gather next to the filter's with the bytes each
reads plus writes per second (2 x the output: every output byte is read once from the lines or the dictionary).

--parent-lib PATH: the condition that plain sets did not get slower.  KeySet creation and lookup_lines on PLAIN sets of the
three sizes are timed in child processes that load PATH (a build of the parent commit, through SREGEX_AMD_LIB) and this
tree's library in turn: parent, branch, parent, branch.  The branch must lie within the spread the two parent runs show.

    python tools/join_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile] [--parent-lib PATH --parent-commit ID] [--box NAME]
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
from lookup_probe import GROUPS, L, NLINES, PATTERN, WIDTH, fill_lines, fill_set, key_columns, timed, upload

SET_SIZES = (1, 4096, NLINES)
VALUES = (1, 4)
VLEN = 8
TAB, NL = 0x09, 0x0A
KERNELS = ("sre_k_keyset_join", "sre_k_keyset_probe", "sre_k_join_gather", "sre_k_lines_gather", "sre_k_extract_select",
           "sre_k_filter_select")


def map_rows(size, nv):
    """the dictionary as an array of rows: key, then nv times a tab and 8 capitals that spell row * 4 + column"""
    a = np.full((size, WIDTH + nv * (VLEN + 1) + 1), NL, dtype=np.uint8)
    r = np.arange(size, dtype=np.int64)
    for j, col in enumerate(key_columns(r)):
        a[:, j] = col
    for c in range(nv):
        at = WIDTH + c * (VLEN + 1)
        a[:, at] = TAB
        v = r * 4 + c
        for j in range(VLEN):
            a[:, at + 1 + j] = ord("A") + (v >> (4 * (VLEN - 1 - j))) % 16
    return a


def host_join(sc, buf, nbytes, ks, out, keyid, index, data, tails):
    """(e): the semi-join on the device, its index and key ids to the host, the rows built in Python"""
    info = sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES, index_ptr=index.ptr,
                           index_cap=NLINES)
    idx = np.frombuffer(index.to_bytes(32 * info.nwritten), dtype=np.int64).reshape(-1, 4)
    kid = np.frombuffer(keyid.to_bytes(8 * NLINES), dtype=np.int64)
    rows = [data[st:st + n] + tails[k] for st, n, k in zip(idx[:, 1].tolist(), idx[:, 2].tolist(), kid[idx[:, 0]].tolist())]
    return b"".join(rows)


def run_map(lib, pool, prog, size, nv, reps):
    a = map_rows(size, nv)
    dbuf, dbytes = upload(lib, a.tobytes())
    tc = []
    for rep in range(reps + 1):
        dt, ks = timed(lambda: S.KeySet(dbuf.ptr, dbytes, 1 + nv, nkeys=1))
        assert (ks.rows, ks.distinct, ks.fields, ks.values) == (size, size, 1, nv)
        if rep:
            tc.append(dt)
        if rep < reps:
            ks.close()
    tails = [bytes(row[WIDTH:]) for row in a]
    buf, nbytes, nmem = fill_lines(lib, size, 100)
    assert nmem == NLINES
    data = buf.to_bytes(nbytes)
    row_bytes = L + nv * (VLEN + 1)
    out, keyid, index = S.DeviceBuffer(NLINES * row_bytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(32 * NLINES)
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    vcols = list(range(nv))
    tj, tl, th = [], [], []
    for rep in range(reps + 1):             # (the first round warms up: code objects, buffers)
        dj, info = timed(lambda: sc.join_lines(buf.ptr, nbytes, out.ptr, NLINES * row_bytes, GROUPS, ks, vcols, keyid_ptr=keyid.ptr,
                                               keyid_cap=NLINES))
        assert sc.last_lines_device == 1
        assert info == S.LookupInfo(NLINES, NLINES, NLINES, NLINES, NLINES * row_bytes, NLINES, NLINES * row_bytes), info
        if rep == 0:
            joined = out.to_bytes(info.out_bytes)
        dl, linfo = timed(lambda: sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES))
        assert linfo == S.LookupInfo(NLINES, NLINES, NLINES, NLINES, nbytes, NLINES, nbytes), linfo
        dh, rows = timed(lambda: host_join(sc, buf, nbytes, ks, out, keyid, index, data, tails))
        assert rows == joined               # the device's rows are the Python join's, byte for byte
        if rep:
            tj.append(dj)
            tl.append(dl)
            th.append(dh)
    res = {"map_keys": size, "value_columns": nv, "map_slots": ks.slots, "map_device_bytes": ks.device_bytes, "lines": NLINES,
           "bytes": nbytes, "out_bytes": NLINES * row_bytes, "kernel": sc.kernel_name, "keymap_create_ms": ms(tc), "join_ms": ms(tj),
           "lookup_ms": ms(tl), "host_lookup_download_python_join_ms": ms(th),
           "join_over_lookup": statistics.median(tj) / statistics.median(tl),
           "join_over_host": statistics.median(tj) / statistics.median(th)}
    for b in (buf, out, keyid, index, dbuf):
        b.free()
    ks.close()
    return res


def child(calls):
    """the run to put under the profiler: `calls` join and lookup calls per configuration after one warm-up call each"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        for size in SET_SIZES:
            buf, nbytes, _ = fill_lines(lib, size, 100)
            for nv in VALUES:
                dbuf, dbytes = upload(lib, map_rows(size, nv).tobytes())
                ks = S.KeySet(dbuf.ptr, dbytes, 1 + nv, nkeys=1)
                cap = NLINES * (L + nv * (VLEN + 1))
                out, keyid = S.DeviceBuffer(cap), S.DeviceBuffer(8 * NLINES)
                for _ in range(calls + 1):
                    sc.join_lines(buf.ptr, nbytes, out.ptr, cap, GROUPS, ks, list(range(nv)), keyid_ptr=keyid.ptr, keyid_cap=NLINES)
                    sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES)
                for b in (out, keyid, dbuf):
                    b.free()
                ks.close()
            buf.free()


def profile(calls, stats_out):
    """(c), (d): the child under rocprofv3; every listed kernel's dispatches in order, per configuration"""
    tmp = tempfile.mkdtemp(prefix="join_probe_")
    configs = [(size, nv) for size in SET_SIZES for nv in VALUES]
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
            all_rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        med = {}
        for name in KERNELS:
            ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in all_rows if name in r["Kernel_Name"]]
            each = len(ns) // len(configs)
            assert each * len(configs) == len(ns) and each % (calls + 1) == 0, (name, len(ns))
            d = each // (calls + 1)             # dispatches of a round
            for i, cfg in enumerate(configs):
                med[(name, cfg)] = (statistics.median(ns[i * each + d:(i + 1) * each]) / 1e3, d)
        per = []
        for size, nv in configs:
            cfg = (size, nv)
            jout, fout = NLINES * (L + nv * (VLEN + 1)), NLINES * L
            jg, fg = med[("sre_k_join_gather", cfg)][0], med[("sre_k_lines_gather", cfg)][0]
            per.append({"map_keys": size, "value_columns": nv,
                        "join_pass_us": med[("sre_k_keyset_join", cfg)][0], "probe_pass_us": med[("sre_k_keyset_probe", cfg)][0],
                        "join_gather_us": jg, "filter_gather_us": fg,
                        "join_gather_GBps_read_plus_written": 2 * jout / jg / 1e3,
                        "filter_gather_GBps_read_plus_written": 2 * fout / fg / 1e3,
                        "extract_select_us": med[("sre_k_extract_select", cfg)][0],
                        "filter_select_us": med[("sre_k_filter_select", cfg)][0]})
        with open(stats[0], newline="") as f:
            top = stats_top(csv.DictReader(f), 20)
        return per, top
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def plain(reps):
    """KeySet creation and lookup_lines on PLAIN sets with whatever library this process loaded"""
    lib = S.load_library()
    res = []
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        for size in SET_SIZES:
            dbuf, dbytes = fill_set(lib, size)
            tc, tl = [], []
            for rep in range(reps + 1):
                dt, ks = timed(lambda: S.KeySet(dbuf.ptr, dbytes, 1))
                if rep:
                    tc.append(dt)
                if rep < reps:
                    ks.close()
            buf, nbytes, _ = fill_lines(lib, size, 100)
            out, keyid = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES)
            for rep in range(reps + 1):
                dl, info = timed(lambda: sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr,
                                                         keyid_cap=NLINES))
                assert info.nwritten == NLINES
                if rep:
                    tl.append(dl)
            res.append({"set_keys": size, "device_bytes": ks.device_bytes, "keyset_create_ms": ms(tc), "lookup_ms": ms(tl)})
            for b in (buf, out, keyid, dbuf):
                b.free()
            ks.close()
    print(json.dumps(res))


def plain_ab(parent_lib, reps):
    """parent, branch, parent, branch in child processes of their own; per size and metric the four medians and whether
    the branch's lie within the spread of the parent's two runs"""
    runs = []
    for which in ("parent", "branch", "parent", "branch"):
        env = dict(os.environ)
        env.pop("SREGEX_AMD_LIB", None)
        if which == "parent":
            env["SREGEX_AMD_LIB"] = parent_lib
        text = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain", "--reps", str(reps)], check=True, env=env,
                              stdout=subprocess.PIPE, timeout=300).stdout.decode()
        runs.append((which, json.loads(text.strip().splitlines()[-1])))
    rows = []
    for i, size in enumerate(SET_SIZES):
        for metric in ("keyset_create_ms", "lookup_ms"):
            p = [r[i][metric]["median"] for w, r in runs if w == "parent"]
            b = [r[i][metric]["median"] for w, r in runs if w == "branch"]
            spread = abs(p[0] - p[1])
            rows.append({"set_keys": size, "metric": metric, "parent_runs_ms": p, "branch_runs_ms": b, "parent_spread_ms": spread,
                         "branch_within_parent_spread": max(b) <= max(p) + spread,
                         "device_bytes_parent": [r[i]["device_bytes"] for w, r in runs if w == "parent"][0],
                         "device_bytes_branch": [r[i]["device_bytes"] for w, r in runs if w == "branch"][0]})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-out", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default=None, help="the commit --parent-lib was built from, for the record")
    ap.add_argument("--box", default=None, help="the name of the machine, for the record")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-calls", type=int, default=5, help=argparse.SUPPRESS)
    ap.add_argument("--plain", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child_calls)
        return
    if args.plain:
        plain(args.reps)
        return
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    doc = {"tool": "tools/join_probe.py", "parent_commit": args.parent_commit, "box": args.box, "reps": args.reps, "lines": NLINES,
           "line_bytes": L, "value_bytes": VLEN,
           "timing": "host clock around each synchronous call; median of reps after a warm-up; join_lines (rows and key ids), "
                     "lookup_lines on the same map (lines and key ids) and lookup_lines with index + download of index and key "
                     "ids + a Python join alternating in one process; every line is a member",
           "pattern": PATTERN.decode(), "groups": GROUPS, "results": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        for size in SET_SIZES:
            for nv in VALUES:
                r = run_map(lib, pool, prog, size, nv, args.reps)
                print(json.dumps(r), flush=True)
                doc["results"].append(r)
    if not args.no_profile:
        per, top = profile(3, args.stats_out)
        doc["kernels"] = {"run": "join_lines and lookup_lines alternating on the same lines and map under rocprofv3 --kernel-trace "
                                 "--stats, in a run of its own: 3 calls of each per configuration after a warm-up call, whose "
                                 "dispatches are left out; medians per dispatch (us); a gather's bytes read plus written are "
                                 "2 x its output",
                          "kernel_stats_top": top, "rows": per}
    if args.parent_lib:
        doc["plain_sets_parent_vs_branch"] = {
            "run": "KeySet creation and lookup_lines on plain sets, every line a member, in child processes that load the parent "
                   "commit's library and this tree's in turn (parent, branch, parent, branch); medians of reps after a warm-up",
            "rows": plain_ab(args.parent_lib, args.reps)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
