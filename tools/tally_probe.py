"""The line tally against the line extract on the same buffer (sre_hip_tally_lines vs sre_hip_extract_lines).

A million 96-byte log lines, each with k=KEY (five letters), the program k=([a-z]+) in mode FIRST on the table-driven
scanner, group [1].  The key of line i is the number i % C in letters, for C = 1, 16, 4096 and one key per line.  Per
cardinality
  (a) the whole tally_lines call (rows, counts and key ids; no index) and
  (b) extract_lines of the same group, which is the call a user makes today before grouping the rows elsewhere,
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after a
warm-up.  Then (c): one run of every cardinality under rocprofv3 --kernel-trace --stats in a child process that makes the
same calls; its kernel statistics go to --stats-out, and the tally's own kernels and the kernels both calls share are
listed per cardinality with their median time per dispatch, the shared ones for each of the two calls.  Prints one JSON
document (--out also writes it to a file).

    python tools/tally_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile]
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
PATTERN = rb"k=([a-z]+)"
GROUPS = [1]
HEAD = b"GET /index.html k="
KERNELS = ("sre_k_tally_insert", "sre_k_tally_keep", "sre_k_tally_ranks", "sre_k_tally_keyid", "sre_k_extract_gather",
           "sre_k_extract_select", "sre_k_filter_sums", "sre_k_filter_offsets")


def key_text(v):
    return bytes(ord("a") + (v // 26 ** (WIDTH - 1 - j)) % 26 for j in range(WIDTH))


def fill_keyed(lib, card):
    """the buffer: line i = HEAD, the key of i % card, a tail of x, a newline"""
    row = np.frombuffer((HEAD + b"a" * WIDTH + b" user nobody " + b"x" * L)[:L - 1] + b"\n", dtype=np.uint8)
    a = np.tile(row, (NLINES, 1))
    v = np.arange(NLINES, dtype=np.int64) % card
    for j in range(WIDTH):
        a[:, len(HEAD) + j] = ord("a") + (v // 26 ** (WIDTH - 1 - j)) % 26
    raw = a.tobytes()
    buf = S.DeviceBuffer(len(raw))
    step = 32 << 20
    for o in range(0, len(raw), step):
        piece = raw[o:o + step]
        assert lib.sre_hip_upload(buf.ptr + o, piece, len(piece)) == 0
    return buf, len(raw)


def time_tally(sc, buf, nbytes, out, cap, counts, keyid):
    t0 = time.perf_counter()
    info = sc.tally_lines(buf.ptr, nbytes, out.ptr, cap, GROUPS, NLINES, counts_ptr=counts.ptr, counts_cap=NLINES,
                          keyid_ptr=keyid.ptr, keyid_cap=NLINES)
    return time.perf_counter() - t0, info


def time_extract(sc, buf, nbytes, out, cap):
    t0 = time.perf_counter()
    info = sc.extract_lines(buf.ptr, nbytes, GROUPS, out.ptr, cap)
    return time.perf_counter() - t0, info


def run_config(lib, pool, prog, card, reps):
    buf, nbytes = fill_keyed(lib, card)
    out, counts, keyid = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(8 * NLINES)
    sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    assert sc.engine == S.ENGINE_SCAN
    tt, te = [], []
    for rep in range(reps + 1):         # (the first round warms up: code objects, buffers)
        dt, info = time_tally(sc, buf, nbytes, out, nbytes, counts, keyid)
        assert sc.last_lines_device == 1
        assert info == S.TallyInfo(NLINES, NLINES, card, card * (WIDTH + 1), card, card * (WIDTH + 1)), info
        de, einfo = time_extract(sc, buf, nbytes, out, nbytes)
        assert einfo.nselected == einfo.nwritten == NLINES and einfo.out_bytes == NLINES * (WIDTH + 1)
        if rep:
            tt.append(dt)
            te.append(de)
    # the first keys and their counts, and the last line's key id
    dt, info = time_tally(sc, buf, nbytes, out, nbytes, counts, keyid)
    k = min(card, 3)
    head = ctypes.create_string_buffer(k * (WIDTH + 1))
    assert lib.sre_hip_download(head, out.ptr, len(head)) == 0
    assert head.raw == b"".join(key_text(v) + b"\n" for v in range(k)), head.raw
    c = (ctypes.c_uint64 * k)()
    assert lib.sre_hip_download(c, counts.ptr, 8 * k) == 0
    assert list(c) == [NLINES // card + (1 if v < NLINES % card else 0) for v in range(k)], list(c)
    last = ctypes.c_int64()
    assert lib.sre_hip_download(ctypes.byref(last), keyid.ptr + 8 * (NLINES - 1), 8) == 0 and last.value == (NLINES - 1) % card
    row = {"keys": card, "lines": NLINES, "bytes": nbytes, "tally_out_bytes": info.out_bytes, "extract_out_bytes": einfo.out_bytes,
           "kernel": sc.kernel_name, "tally_ms": ms(tt), "extract_ms": ms(te),
           "tally_over_extract": statistics.median(tt) / statistics.median(te)}
    for b in (buf, out, counts, keyid):
        b.free()
    return row


def child(cards, calls):
    """the run to put under the profiler: `calls` tally and extract calls per cardinality after one warm-up call each"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        for card in cards:
            buf, nbytes = fill_keyed(lib, card)
            out, counts, keyid = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(8 * NLINES)
            for _ in range(calls + 1):
                time_tally(sc, buf, nbytes, out, nbytes, counts, keyid)
                time_extract(sc, buf, nbytes, out, nbytes)
            for b in (buf, out, counts, keyid):
                b.free()


def profile(cards, calls, stats_out):
    """(c): the child under rocprofv3; every listed kernel's dispatches in order, per cardinality"""
    tmp = tempfile.mkdtemp(prefix="tally_probe_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", ",".join(str(c) for c in cards), "--child-calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=400)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert stats and trace, os.listdir(tmp)
        if stats_out:
            shutil.copyfile(stats[0], stats_out)
        with open(trace[0], newline="") as f:
            all_rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        per = []
        for name in KERNELS:
            ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in all_rows if name in r["Kernel_Name"]]
            each = len(ns) // len(cards)
            assert each * len(cards) == len(ns) and each % (calls + 1) == 0, (name, len(ns))
            d = each // (calls + 1)             # dispatches of a round: the tally call's, then the extract call's
            for i, card in enumerate(cards):
                mine = ns[i * each + d:(i + 1) * each]
                row = {"kernel": name, "keys": card, "dispatches_per_round": d}
                if name.startswith("sre_k_tally"):
                    row["median_us"] = statistics.median(mine) / 1e3
                else:
                    assert d % 2 == 0, (name, d)
                    row["tally_median_us"] = statistics.median(x for j, x in enumerate(mine) if j % d < d // 2) / 1e3
                    row["extract_median_us"] = statistics.median(x for j, x in enumerate(mine) if j % d >= d // 2) / 1e3
                per.append(row)
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
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-calls", type=int, default=5, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        child([int(c) for c in args.child.split(",")], args.child_calls)
        return
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    doc = {"tool": "tools/tally_probe.py", "commit": commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps after a warm-up, tally_lines (rows, counts, key ids; "
                     "max_keys = lines) and extract_lines of the same group alternating in one process",
           "pattern": PATTERN.decode(), "groups": GROUPS, "results": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        for card in CARDINALITIES:
            r = run_config(lib, pool, prog, card, args.reps)
            print(json.dumps(r), flush=True)
            doc["results"].append(r)
    if not args.no_profile:
        per, top = profile(list(CARDINALITIES), 5, args.stats_out)
        doc["kernels"] = {"run": "tally_lines and extract_lines alternating on the same lines under rocprofv3 --kernel-trace --stats, "
                                 "5 calls of each per cardinality after a warm-up call; per kernel the dispatches of the warm-up "
                                 "round are left out",
                          "kernel_stats_top": top, "rows": per}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
