"""The line tally with sums against the plain tally, and against what a caller pays without it
(sre_hip_tally_sums_lines vs sre_hip_tally_lines vs tally + extract + download + numpy).

A million 96-byte log lines, each with k=KEY;v=DDDDDD;w=DDDD;x=DDD;y=DD (KEY five letters, the numbers zero-padded), the
program k=([a-z]+);v=([0-9]+);w=([0-9]+);x=([0-9]+);y=([0-9]+) in mode FIRST on the table-driven scanner, key group [1].
The key of line i is the number i % C in letters, for C = 1, 16, 4096 and one key per line; the value columns are group 2
(V = 1) or groups 2 .. 5 (V = 4).  Per cardinality and V
  (a) the whole tally_sums_lines call (rows, counts, key ids, sums; no index),
  (b) tally_lines with the same arguments, and
  (c) what a caller pays today: tally_lines for the key ids, extract_lines of the value groups with its index, a download
      of the key ids and of the extract's rows, and a numpy parse and reduction (sum, min, max per key).  The parse knows
      that the fields of this buffer have fixed widths and reads the rows, not the index: (c) flatters the caller
alternate in one process, each timed by the host clock around the synchronous calls: the median of --reps rounds after a
warm-up.  Then one run of every configuration under rocprofv3 --kernel-trace --stats in a child process that makes the
calls (a) and (b); its kernel statistics go to --stats-out, and the new kernels and the select pass are listed per
configuration with their median time per dispatch.  With --parent-lib, tally_lines alone is timed in child processes
(--tally-only), alternating: that library (a build of the parent commit, --parent-commit names it), this one, and both
again; the two runs of each give the run-to-run spread.  Prints one JSON document (--out also writes it to a file).

    python tools/tally_sums_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile] [--parent-lib libsregex.so --parent-commit HASH]
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
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sregex_amd as S
from filter_probe import ms
from extract_probe import stats_top

NLINES = 1 << 20
L = 96
WIDTH = 5                                   # letters of a key: 26^5 > NLINES
CARDINALITIES = (1, 16, 4096, NLINES)
COLUMNS = (1, 4)
PATTERN = rb"k=([a-z]+);v=([0-9]+);w=([0-9]+);x=([0-9]+);y=([0-9]+)"
GROUPS = [1]
VGROUPS = [2, 3, 4, 5]
DIGITS = (6, 4, 3, 2)
HEAD = b"GET /index.html k="
KERNELS = ("sre_k_tally_sums_init", "sre_k_tally_sums", "sre_k_tally_sums_merge", "sre_k_extract_select", "sre_k_tally_insert", "sre_k_tally_ranks")


def values(c):
    """the number of every line in value column c"""
    i = np.arange(NLINES, dtype=np.int64)
    return (i * (7919, 31, 7, 3)[c] + c) % 10 ** DIGITS[c]


def fill_keyed(lib, card):
    """the buffer: line i = HEAD, the key of i % card, the four numbers, a tail of x, a newline"""
    text = HEAD + b"a" * WIDTH + b"".join(b";" + b"vwxy"[c:c + 1] + b"=" + b"0" * DIGITS[c] for c in range(4))
    row = np.frombuffer((text + b" user nobody " + b"x" * L)[:L - 1] + b"\n", dtype=np.uint8)
    a = np.tile(row, (NLINES, 1))
    v = np.arange(NLINES, dtype=np.int64) % card
    for j in range(WIDTH):
        a[:, len(HEAD) + j] = ord("a") + (v // 26 ** (WIDTH - 1 - j)) % 26
    at = len(HEAD) + WIDTH
    for c in range(4):
        at += 3
        x = values(c)
        for j in range(DIGITS[c]):
            a[:, at + j] = ord("0") + (x // 10 ** (DIGITS[c] - 1 - j)) % 10
        at += DIGITS[c]
    raw = a.tobytes()
    buf = S.DeviceBuffer(len(raw))
    step = 32 << 20
    for o in range(0, len(raw), step):
        piece = raw[o:o + step]
        assert lib.sre_hip_upload(buf.ptr + o, piece, len(piece)) == 0
    return buf, len(raw)


class Buffers:
    def __init__(self, nbytes, index_width):
        self.out, self.counts, self.keyid = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(8 * NLINES)
        self.sums = S.DeviceBuffer(32 * len(VGROUPS) * NLINES)
        self.index = S.DeviceBuffer(8 * index_width * NLINES)
        self.cap = nbytes

    def free(self):
        for b in (self.out, self.counts, self.keyid, self.sums, self.index):
            b.free()


def time_sums(sc, buf, nbytes, b, nv):
    t0 = time.perf_counter()
    info = sc.tally_sums_lines(buf.ptr, nbytes, b.out.ptr, b.cap, GROUPS, VGROUPS[:nv], NLINES, counts_ptr=b.counts.ptr,
                               counts_cap=NLINES, sums_ptr=b.sums.ptr, sums_cap=NLINES, keyid_ptr=b.keyid.ptr, keyid_cap=NLINES)
    return time.perf_counter() - t0, info


def time_tally(sc, buf, nbytes, b):
    t0 = time.perf_counter()
    info = sc.tally_lines(buf.ptr, nbytes, b.out.ptr, b.cap, GROUPS, NLINES, counts_ptr=b.counts.ptr, counts_cap=NLINES,
                          keyid_ptr=b.keyid.ptr, keyid_cap=NLINES)
    return time.perf_counter() - t0, info


def time_today(lib, sc, buf, nbytes, b, nv, nkeys):
    """(c): key ids from the tally, the value fields from the extract, both downloaded, parsed and reduced with numpy"""
    t0 = time.perf_counter()
    sc.tally_lines(buf.ptr, nbytes, None, 0, GROUPS, NLINES, keyid_ptr=b.keyid.ptr, keyid_cap=NLINES)
    keyid = np.empty(NLINES, dtype=np.int64)
    assert lib.sre_hip_download(keyid.ctypes.data, b.keyid.ptr, keyid.nbytes) == 0
    einfo = sc.extract_lines(buf.ptr, nbytes, VGROUPS[:nv], b.out.ptr, b.cap, index_ptr=b.index.ptr, index_cap=NLINES)
    rows = np.empty(einfo.out_bytes, dtype=np.uint8)
    assert lib.sre_hip_download(rows.ctypes.data, b.out.ptr, rows.nbytes) == 0
    rows = rows.reshape(NLINES, -1)
    res, at = [], 0
    for c in range(nv):
        x = np.zeros(NLINES, dtype=np.int64)
        for j in range(DIGITS[c]):
            x = x * 10 + (rows[:, at + j].astype(np.int64) - ord("0"))
        at += DIGITS[c] + 1
        s, lo, hi = np.zeros(nkeys, dtype=np.int64), np.full(nkeys, np.iinfo(np.int64).max), np.full(nkeys, np.iinfo(np.int64).min)
        np.add.at(s, keyid, x)
        np.minimum.at(lo, keyid, x)
        np.maximum.at(hi, keyid, x)
        res.append((s, lo, hi))
    return time.perf_counter() - t0, res


def download_sums(lib, b, nkeys, nv):
    a = np.empty((nkeys, nv, 4), dtype=np.int64)
    assert lib.sre_hip_download(a.ctypes.data, b.sums.ptr, a.nbytes) == 0
    return a


def run_config(lib, pool, prog, card, nv, reps):
    buf, nbytes = fill_keyed(lib, card)
    b = Buffers(nbytes, 4 + 2 * nv)
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    ta, tb, tc = [], [], []
    want = S.TallyInfo(NLINES, NLINES, card, card * (WIDTH + 1), card, card * (WIDTH + 1))
    today = None
    for rep in range(reps + 1):         # (the first round warms up: code objects, buffers)
        da, info = time_sums(sc, buf, nbytes, b, nv)
        assert sc.last_lines_device == 1 and info == want, info
        db, info = time_tally(sc, buf, nbytes, b)
        assert info == want, info
        dc, today = time_today(lib, sc, buf, nbytes, b, nv, card)
        if rep:
            ta.append(da)
            tb.append(db)
            tc.append(dc)
    # the device's aggregates are numpy's
    time_sums(sc, buf, nbytes, b, nv)
    got = download_sums(lib, b, card, nv)
    per_key = np.bincount(np.arange(NLINES) % card, minlength=card)
    for c in range(nv):
        s, lo, hi = today[c]
        assert (got[:, c, 0] == s).all() and (got[:, c, 1] == lo).all() and (got[:, c, 2] == hi).all(), (card, nv, c)
        assert (got[:, c, 3] == per_key).all()
    a, bb, cc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    row = {"keys": card, "columns": nv, "lines": NLINES, "bytes": nbytes, "kernel": sc.kernel_name, "sums_ms": ms(ta),
           "tally_ms": ms(tb), "today_ms": ms(tc), "sums_minus_tally_us": (a - bb) * 1e6, "sums_over_tally": a / bb,
           "sums_over_today": a / cc}
    buf.free()
    b.free()
    return row


def tally_only(reps):
    """(b) alone, for a library that may lack the sums (SREGEX_AMD_LIB): the median per cardinality"""
    lib = S.load_library()
    out = {}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        for card in CARDINALITIES:
            buf, nbytes = fill_keyed(lib, card)
            b = Buffers(nbytes, 1)
            sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
            ts = [time_tally(sc, buf, nbytes, b)[0] for _ in range(reps + 1)][1:]
            out[str(card)] = ms(ts)
            buf.free()
            b.free()
    print(json.dumps(out))


def tally_only_child(lib_path, reps):
    env = dict(os.environ)
    if lib_path:
        env["SREGEX_AMD_LIB"] = os.path.abspath(lib_path)
    else:
        env.pop("SREGEX_AMD_LIB", None)
    text = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--tally-only", "--reps", str(reps)], env=env,
                                   timeout=300)
    return json.loads(text.decode().strip().splitlines()[-1])


def child(cards, calls):
    """the run to put under the profiler: `calls` sums and tally calls per configuration after one warm-up call each"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        for card in cards:
            buf, nbytes = fill_keyed(lib, card)
            b = Buffers(nbytes, 1)
            for nv in COLUMNS:
                for _ in range(calls + 1):
                    time_sums(sc, buf, nbytes, b, nv)
                    time_tally(sc, buf, nbytes, b)
            buf.free()
            b.free()


def profile(cards, calls, stats_out):
    """the child under rocprofv3; every listed kernel's dispatches in order, per configuration"""
    tmp = tempfile.mkdtemp(prefix="tally_sums_probe_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", ",".join(str(c) for c in cards), "--child-calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=360)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert stats and trace, os.listdir(tmp)
        if stats_out:
            shutil.copyfile(stats[0], stats_out)
        with open(trace[0], newline="") as f:
            all_rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        configs = [(card, nv) for card in cards for nv in COLUMNS]
        per = []
        for name in KERNELS:
            ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in all_rows
                  if name in r["Kernel_Name"] and (name != "sre_k_tally_sums" or "sre_k_tally_sums_" not in r["Kernel_Name"])]
            # (the merge runs only where the waves send to copies: sre_ls_copies, 8 MiB over the bytes of the rows)
            mine_configs = [c for c in configs if name != "sre_k_tally_sums_merge" or (8 << 20) // (c[0] * c[1] * 32) > 1]
            each = len(ns) // len(mine_configs)
            assert each * len(mine_configs) == len(ns) and each % (calls + 1) == 0, (name, len(ns))
            d = each // (calls + 1)             # dispatches of a round: the sums call's, then the tally call's
            for i, (card, nv) in enumerate(mine_configs):
                mine = ns[i * each + d:(i + 1) * each]
                per.append({"kernel": name, "keys": card, "columns": nv, "dispatches_per_round": d,
                            "median_us": statistics.median(mine) / 1e3, "max_us": max(mine) / 1e3})
        with open(stats[0], newline="") as f:
            top = stats_top(csv.DictReader(f), 20)
        return per, top
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-out", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="a libsregex.so built from the parent commit")
    ap.add_argument("--parent-commit", default=None, help="that commit, for the record (a tree without git history cannot tell)")
    ap.add_argument("--tally-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-calls", type=int, default=5, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        child([int(c) for c in args.child.split(",")], args.child_calls)
        return
    if args.tally_only:
        tally_only(args.reps)
        return
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    doc = {"tool": "tools/tally_sums_probe.py", "commit": commit, "parent_commit": args.parent_commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around the synchronous calls; median of reps after a warm-up; (a) tally_sums_lines (rows, counts, "
                     "key ids, sums; max_keys = lines), (b) tally_lines with the same arguments, (c) tally_lines for key ids + "
                     "extract_lines of the value groups with its index + download of key ids and rows + numpy parse and "
                     "reduction, alternating in one process",
           "pattern": PATTERN.decode(), "groups": GROUPS, "vgroups": VGROUPS, "results": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        for card in CARDINALITIES:
            for nv in COLUMNS:
                r = run_config(lib, pool, prog, card, nv, args.reps)
                print(json.dumps(r), flush=True)
                doc["results"].append(r)
    if args.parent_lib:
        # parent, this, parent, this: a drift of the box over the four runs shows in both pairs alike
        runs = [tally_only_child(args.parent_lib if q % 2 == 0 else None, args.reps) for q in range(4)]
        rows = []
        for card in CARDINALITIES:
            p0, h0, p1, h1 = (r[str(card)]["median"] for r in runs)
            rows.append({"keys": card, "parent_ms": [p0, p1], "parent_spread_ms": abs(p0 - p1), "this_ms": [h0, h1],
                         "this_spread_ms": abs(h0 - h1), "this_mean_minus_parent_mean_ms": (h0 + h1) / 2 - (p0 + p1) / 2})
        doc["tally_lines_against_parent"] = {
            "run": "tally_lines alone in a child process per library, in the order parent, this, parent, this (the parent "
                   "commit's build and this commit's); median of reps after a warm-up per cardinality", "rows": rows}
        print(json.dumps(doc["tally_lines_against_parent"]), flush=True)
    if not args.no_profile:
        per, top = profile(list(CARDINALITIES), 5, args.stats_out)
        doc["kernels"] = {"run": "tally_sums_lines and tally_lines alternating on the same lines under rocprofv3 --kernel-trace "
                                 "--stats, 5 calls of each per configuration after a warm-up call; per kernel the dispatches of "
                                 "the warm-up round are left out",
                          "kernel_stats_top": top, "rows": per}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
